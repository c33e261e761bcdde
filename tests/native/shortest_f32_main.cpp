// Stand-alone driver of oarfish_amd/csrc/oem_shortest_f32.h for tests/test_shortest_f32.py (host compiler, sanitizers on).
//
//   shortest_f32_main            stdin, one f32 bit pattern (hex) per line; stdout, per line:
//                                <the emitted text> <the measured length>
//                                Each text is emitted into a heap block of exactly the measured length: a printer that
//                                writes more than it measured trips the sanitizer.
//   shortest_f32_main --sweep S  self-checks that need no reference, over the positive finite bit patterns 1, 1 + S,
//                                1 + 2 S, ... and over the patterns named below; prints one summary line, exits 1 at the
//                                first violation:
//                                  * strtof(text) has the same bits;
//                                  * at most 9 significant digits;
//                                  * with one digit fewer, neither the truncated nor the rounded-up candidate reads
//                                    back as the same bits (so the text is shortest);
//                                  * no text is longer than the header's bound, and the bound is attained;
//                                  * (where <charconv> prints floats) the digits and the decimal exponent are those of
//                                    std::to_chars' shortest scientific form.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#if __has_include(<charconv>)
#include <charconv>
#endif

#include "../../oarfish_amd/csrc/oem_shortest_f32.h"

#if defined(__cpp_lib_to_chars) && __cpp_lib_to_chars >= 201611L
#define HAVE_FLOAT_TO_CHARS 1
#else
#define HAVE_FLOAT_TO_CHARS 0
#endif

namespace {

uint32_t bits_of(float x)
{
    uint32_t b;
    memcpy(&b, &x, sizeof b);
    return b;
}

// the text of `bits` in a block of exactly the measured size
std::string text_of(uint32_t bits, uint32_t *measured)
{
    const uint32_t n = oem::shortest_f32_len(bits);
    std::unique_ptr<uint8_t[]> buf(new uint8_t[n ? n : 1]);
    const uint8_t *end = oem::emit_shortest_f32(buf.get(), bits);
    *measured = n;
    return std::string((const char *)buf.get(), (size_t)(end - buf.get()));
}

uint32_t parse_bits(const char *s)
{
    return bits_of(strtof(s, nullptr));
}

// digits (no trailing zero) and exponent of the text's value: text = digits * 10^exp10
void digits_of(const std::string &t, uint64_t *digits, int *n_digits, int *exp10)
{
    std::string d;
    int frac = 0;
    bool seen_point = false;
    for (char ch : t) {
        if (ch == '.') {
            seen_point = true;
            continue;
        }
        d.push_back(ch);
        if (seen_point) ++frac;
    }
    size_t first = d.find_first_not_of('0');
    d = d.substr(first);
    int e = -frac;
    while (d.size() > 1 && d.back() == '0') {
        d.pop_back();
        ++e;
    }
    *digits = strtoull(d.c_str(), nullptr, 10);
    *n_digits = (int)d.size();
    *exp10 = e;
}

int fail_at(uint32_t bits, const char *what, const std::string &text)
{
    fprintf(stderr, "0x%08x: %s (text %s)\n", bits, what, text.c_str());
    return 1;
}

int check_one(uint32_t bits, uint32_t *longest)
{
    uint32_t n = 0;
    const std::string t = text_of(bits, &n);
    if (t.size() != n) return fail_at(bits, "measured length differs from the emitted length", t);
    if (n > *longest) *longest = n;
    if (parse_bits(t.c_str()) != bits) return fail_at(bits, "strtof does not read the text back", t);
    uint64_t d;
    int nd, e;
    digits_of(t, &d, &nd, &e);
    if (nd > 9) return fail_at(bits, "more than 9 significant digits", t);
    if (nd > 1) {
        char cand[64];
        for (uint64_t c : {d / 10, d / 10 + 1}) {
            snprintf(cand, sizeof cand, "%" PRIu64 "e%d", c, e + 1);
            if (parse_bits(cand) == bits) return fail_at(bits, (std::string("a shorter decimal reads back the same: ") + cand).c_str(), t);
        }
    }
#if HAVE_FLOAT_TO_CHARS
    {
        float x;
        memcpy(&x, &bits, sizeof x);
        char sci[64];
        const auto r = std::to_chars(sci, sci + sizeof sci - 1, x, std::chars_format::scientific);
        *r.ptr = 0;
        // d.ddddde[+-]XX
        std::string ds;
        const char *p = sci;
        for (; *p && *p != 'e'; ++p)
            if (*p != '.') ds.push_back(*p);
        const int sci_e = atoi(p + 1);
        while (ds.size() > 1 && ds.back() == '0') ds.pop_back();
        if (strtoull(ds.c_str(), nullptr, 10) != d || sci_e - ((int)ds.size() - 1) != e)
            return fail_at(bits, (std::string("std::to_chars prints ") + sci).c_str(), t);
    }
#endif
    return 0;
}

int sweep(uint32_t stride)
{
    uint32_t longest = 0;
    uint64_t n = 0;
    for (uint64_t b = 1; b < 0x7f800000ull; b += stride, ++n)
        if (check_one((uint32_t)b, &longest)) return 1;
    // every edge of the format, whatever the stride: the ends of the subnormals, of the normals, powers of two
    for (uint32_t b : {0x00000001u, 0x007fffffu, 0x00800000u, 0x00800001u, 0x7f7fffffu, 0x7f7ffffeu, 0x3f800000u, 0x4b800000u})
        if (check_one(b, &longest)) return 1;
    // the bound is taken among the smallest subnormals, whose last digit stands at 10^-45: `0.`, 44 zeros, `1`
    uint32_t at_bound = 0;
    for (uint32_t b = 1u; b <= 1000u; ++b) {
        uint32_t l = 0;
        if (check_one(b, &l)) return 1;
        if (l > longest) longest = l;
        if (l + 1 == oem::kShortestF32MaxLen) {
            ++at_bound;
            uint32_t m = 0;
            const std::string neg = text_of(b | 0x80000000u, &m); // ... and a sign
            if (m != oem::kShortestF32MaxLen || neg.size() != m || neg[0] != '-') return fail_at(b, "the negative is not one byte longer", neg);
        }
    }
    if (longest + 1 != oem::kShortestF32MaxLen || at_bound == 0) {
        fprintf(stderr, "longest positive text %u, header's bound %u less the sign, %u patterns at it\n", longest,
                oem::kShortestF32MaxLen, at_bound);
        return 1;
    }
    printf("checked %" PRIu64 " longest %u at_bound %u to_chars %d\n", n, longest, at_bound, HAVE_FLOAT_TO_CHARS);
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "--sweep")) return sweep((uint32_t)strtoul(argv[2], nullptr, 10));
    char line[64];
    while (fgets(line, sizeof line, stdin)) {
        char *end = nullptr;
        const unsigned long b = strtoul(line, &end, 16);
        if (end == line || b > 0xfffffffful) {
            fprintf(stderr, "bad request: %s", line);
            return 2;
        }
        uint32_t n = 0;
        const std::string t = text_of((uint32_t)b, &n);
        printf("%s %u\n", t.c_str(), n);
    }
    return 0;
}
