// oem_collate_device.h -- the resident form of the name collation (oem_collate_device.hip): one batch of cells collated
// on the device, its order and offsets LEFT there.  oem_collate_names copies them to the caller's arrays;
// oem_em_run_cells_records_names_sparse (oem_cells_records.hip) gathers and filters the records behind them instead.
#pragma once

#include "oem_collate.h"
#include "oem_driver.h"

namespace oem {

// One call's input, as oem_collate_names takes it (already checked), and how the batches are run.
struct CollateInput {
    const char *who = nullptr;   // for the messages of the device-found errors
    const uint8_t *names = nullptr;
    const uint64_t *name_off = nullptr;
    const uint8_t *secondary = nullptr;
    const uint64_t *cell_rec_off = nullptr;
    uint32_t mode = kCollateSort;
    uint64_t chunk_bytes = 0;    // name bytes per upload chunk
    bool timing = false;
};

// What a batch leaves on the device.  The batch holds the cells [c0, c1) and their m records.
struct CollateResident {
    DevBuf<uint32_t> order;          // m: order[k] = order_base + the record of the batch at position k
    DevBuf<uint64_t> group_off;      // m + 1 allocated, n_groups + 1 filled: pos_base + the positions where a read starts, then pos_base + m
    DevBuf<uint64_t> cell_group_off; // (c1 - c0) + 1: group_base + the cells' first groups
    uint64_t n_groups = 0;
};

// The cells [c0, c1) of the call, m > 0 records.  The bases are added on the device: oem_collate_names passes the batch's
// place in the call for all three, a caller that goes on working on the batch passes 0 for the positions and groups.  A
// name error names the record by its index in the call, whatever the bases.  info (8 doubles, collate_last_call's
// layout) is accumulated.  Returns with the device idle and the scratch of the sort released.
int collate_resident(const CollateInput &in, uint32_t c0, uint32_t c1, uint64_t order_base, uint64_t pos_base, uint64_t group_base,
                     double *info, CollateResident *out);

uint64_t collate_chunk_bytes();   // the upload chunk (testing build: OEM_COLLATE_CHUNK_BYTES)
uint64_t collate_batch_records(); // records per batch of oem_collate_names (testing build: OEM_COLLATE_BATCH_RECORDS)
constexpr uint64_t kCollateMaxBatch = (1ull << 31) - 2; // a single cell beyond this is refused (the scans take m + 1 items as an int)

// The argument checks of oem_collate_names on the input side, before any device use.
int check_collate_input(const char *who, const uint8_t *names, const uint64_t *name_off, uint64_t n_records, const uint64_t *cell_rec_off,
                        uint32_t n_cells, uint32_t mode);

} // namespace oem
