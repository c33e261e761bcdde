// Stand-alone host program over the gene rule of oarfish_amd/csrc/oem_gene_counts.h (tests/test_gene_counts.py builds
// it with the address and undefined-behaviour sanitizers).  Cases on stdin, one answer line each:
//   G n_cells nnz n_txps
//   then the n_cells + 1 entries of cell_off, nnz pairs  col value_bits  (the f32 as its u32 bit pattern) and the n_txps
//   entries of gene_of
//       -> ok | counts | genes | value_bits
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../oarfish_amd/csrc/oem_gene_counts.h"

template <typename V>
static void put(const V &v)
{
    printf(" |");
    for (size_t i = 0; i < v.size(); ++i) printf(" %" PRIu64, (uint64_t)v[i]);
}

int main()
{
    char cmd[8];
    while (scanf("%7s", cmd) == 1) {
        if (cmd[0] != 'G') return 2;
        uint32_t n_cells, n_txps;
        uint64_t nnz;
        if (scanf("%" SCNu32 " %" SCNu64 " %" SCNu32, &n_cells, &nnz, &n_txps) != 3) return 2;
        // exactly the entries of every array: one read past them is a sanitizer report
        std::vector<uint64_t> cell_off((size_t)n_cells + 1);
        std::vector<uint32_t> col(nnz), bits(nnz), gene_of(n_txps);
        std::vector<float> val(nnz);
        for (auto &v : cell_off)
            if (scanf("%" SCNu64, &v) != 1) return 2;
        for (uint64_t i = 0; i < nnz; ++i)
            if (scanf("%" SCNu32 " %" SCNu32, &col[i], &bits[i]) != 2) return 2;
        for (auto &v : gene_of)
            if (scanf("%" SCNu32, &v) != 1) return 2;
        if (nnz) memcpy(val.data(), bits.data(), sizeof(float) * nnz);
        std::vector<uint32_t> counts, genes;
        std::vector<float> sums;
        oem::gene_counts_host(cell_off.data(), n_cells, col.data(), val.data(), gene_of.data(), &counts, &genes, &sums);
        std::vector<uint32_t> out_bits(sums.size());
        if (!sums.empty()) memcpy(out_bits.data(), sums.data(), sizeof(float) * sums.size());
        printf("ok");
        put(counts);
        put(genes);
        put(out_bits);
        putchar('\n');
    }
    return 0;
}
