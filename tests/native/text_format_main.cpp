// Stand-alone driver of oarfish_amd/csrc/oem_text_format.h for tests/test_text_format.py (host compiler, sanitizers on).
// stdin, one request per line:   f <bits of an f64, hex> <decimals>   |   u <u32, decimal>   |   U <u64, decimal>
// stdout, one answer per line:   <the emitted text> <the measured length>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../oarfish_amd/csrc/oem_text_format.h"

int main()
{
    char kind;
    unsigned long long a;
    unsigned d;
    char line[128];
    while (fgets(line, sizeof line, stdin)) {
        uint32_t want = 0;
        // exactly the measured number of bytes: a printer that writes more than it measured trips the sanitizer
        std::vector<uint8_t> buf;
        const uint8_t *end = nullptr;
        if (sscanf(line, " %c %llx %u", &kind, &a, &d) == 3 && kind == 'f') {
            double x;
            const uint64_t bits = a;
            memcpy(&x, &bits, sizeof x);
            want = oem::fixed_len(x, d);
            buf.resize(want);
            end = oem::emit_fixed(buf.data(), x, d);
        } else if (sscanf(line, " %c %llu", &kind, &a) == 2 && kind == 'u') {
            want = oem::u32_dec_len((uint32_t)a);
            buf.resize(want);
            end = oem::emit_u32(buf.data(), (uint32_t)a);
        } else if (sscanf(line, " %c %llu", &kind, &a) == 2 && kind == 'U') {
            want = oem::u64_dec_len(a);
            buf.resize(want);
            end = oem::emit_u64(buf.data(), a);
        } else {
            fprintf(stderr, "bad request: %s", line);
            return 2;
        }
        fwrite(buf.data(), 1, (size_t)(end - buf.data()), stdout);
        printf(" %u\n", want);
    }
    return 0;
}
