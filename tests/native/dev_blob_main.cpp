// The growth rule and the allocation sizes of the sessions' device arena (oarfish_amd/csrc/oem_dev_blob.h), without a
// device: the header's host part is plain arithmetic.  tests/test_dev_blob.py builds this under AddressSanitizer + UBSan.
// Prints one "ok <scenario>" line per scenario; the first failed check ends the program with status 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../oarfish_amd/csrc/oem_dev_blob.h"

using namespace oem;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

// the floors of the instances: the sorting arena and the labels, the cells arena, the testing library's knobs
static const uint64_t kFloors[] = {1024, 4096, 1ull << 12, 64ull << 10, 1};

int main()
{
    // need below, at and above 2 * cap: geometric until one append asks for more
    for (uint64_t cap : {1ull, 7ull, 1024ull, 4096ull, 100000ull}) {
        for (uint64_t first : kFloors) {
            if (first > cap) continue; // (a capacity is never below its floor once it is not 0)
            CHECK(next_cap(cap, cap + 1, first) == 2 * cap);
            CHECK(next_cap(cap, 2 * cap - 1, first) == 2 * cap);
            CHECK(next_cap(cap, 2 * cap, first) == 2 * cap);
            CHECK(next_cap(cap, 2 * cap + 1, first) == 2 * cap + 1);
            CHECK(next_cap(cap, 10 * cap + 3, first) == 10 * cap + 3);
        }
    }
    puts("ok need against twice the capacity");

    // the first allocation: the floor, or the need where one append is larger
    for (uint64_t first : kFloors) {
        CHECK(next_cap(0, 1, first) == first);
        CHECK(next_cap(0, first, first) == first);
        CHECK(next_cap(0, first + 1, first) == first + 1);
        CHECK(next_cap(0, 0, first) == first); // an empty blob is allocated all the same
    }
    puts("ok the first capacity with each floor");

    // need == 0 never shrinks, and the result always holds the need
    for (uint64_t cap : {0ull, 1ull, 5ull, 4096ull})
        for (uint64_t first : kFloors) {
            CHECK(next_cap(cap, 0, first) >= cap && next_cap(cap, 0, first) >= first);
            for (uint64_t need : {0ull, 1ull, 17ull, 8191ull, 8192ull, 8193ull}) CHECK(next_cap(cap, need, first) >= need);
        }
    puts("ok need of 0");

    // floors of 1: the capacities of a session that appends one 3-byte item at a time, as the growth test drives it
    {
        uint64_t cap = 0, bytes_cap = 0, n = 0, bytes = 0, grown = 0;
        for (int k = 0; k < 40; ++k) {
            if (n + 1 > cap) {
                cap = next_cap(cap, n + 1, 1);
                ++grown;
            }
            if (bytes + 3 > bytes_cap) bytes_cap = next_cap(bytes_cap, bytes + 3, 1);
            ++n;
            bytes += 3;
            CHECK(cap >= n && bytes_cap >= bytes && cap < 2 * n + 1 && bytes_cap < 2 * bytes + 1);
        }
        CHECK(cap == 64 && grown == 7); // 1, 2, 4, ..., 64
    }
    puts("ok floors of 1");

    // what a capacity allocates: 16 bytes behind a blob's bytes, one offset more than items, 8 bytes behind the flags;
    // the padding that is kept zero lies inside the allocation wherever the used part ends
    for (uint64_t cap : {0ull, 1ull, 15ull, 16ull, 17ull, 4096ull}) {
        CHECK(blob_alloc_bytes(cap) == cap + 16 && blob_alloc_offsets(cap) == cap + 1 && flags_alloc_bytes(cap) == cap + 8);
        std::vector<unsigned char> blob(blob_alloc_bytes(cap), 0xff), flags(flags_alloc_bytes(cap), 0xff);
        std::vector<uint64_t> off(blob_alloc_offsets(cap), ~0ull);
        for (uint64_t used = 0; used <= cap; ++used) {
            CHECK(used + kBlobPad <= blob.size() && used + kFlagPad <= flags.size() && used < off.size());
            for (uint64_t k = 0; k < kBlobPad; ++k) blob[used + k] = 0;
            for (uint64_t k = 0; k < kFlagPad; ++k) flags[used + k] = 0;
            off[used] = used;
        }
        // a full blob: its padding ends where the allocation ends, its last offset is the last entry
        CHECK(cap + kBlobPad == blob.size() && cap + kFlagPad == flags.size() && cap + 1 == off.size());
        CHECK(blob.back() == 0 && flags.back() == 0 && off.back() == cap);
    }
    puts("ok allocation sizes");
    return 0;
}
