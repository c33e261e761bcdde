// Stand-alone driver of oarfish_amd/csrc/oem_shortest_f64.h for tests/test_shortest_f64.py (host compiler, sanitizers on).
//
//   shortest_f64_main            stdin, one f64 bit pattern (hex) per line; stdout, per line:
//                                <the emitted text> <the measured length>
//                                Each text is emitted into a heap block of exactly the measured length: a printer that
//                                writes more than it measured trips the sanitizer.
//   shortest_f64_main --sweep N SEED
//                                self-checks that need no reference, over the patterns named below and N random finite
//                                bit patterns drawn from SEED; prints one summary line, exits 1 at the first violation:
//                                  * the measured length is the emitted length;
//                                  * strtod(text) has the same bits;
//                                  * at most 17 significant digits;
//                                  * with one digit fewer, neither the truncated nor the rounded-up candidate reads
//                                    back as the same bits (so the text is shortest);
//                                  * the digits and the decimal exponent are those of std::to_chars' shortest form,
//                                    and the text is those digits put positionally;
//                                  * no text is longer than the header's bound, and the bound is attained.
//                                The named patterns: every power of two and every power of ten in range, each with its
//                                two neighbours (the powers of two are the boundary cases of a shortest-digit
//                                algorithm: the interval below them is half as wide); 5e-324, the largest subnormal,
//                                the smallest normal, DBL_MAX; 2^53 - 1, 2^53, 2^53 + 2 (the neighbours of the integer
//                                2^53 + 1 = 9007199254740993, which is no f64 and reads as 2^53); 0.1 + 0.2; 1e21,
//                                1e22, 1e23; +0 and -0; and published hard cases of shortest-digit printers.
#include <cfloat>
#include <cmath>
#include <charconv>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../oarfish_amd/csrc/oem_shortest_f64.h"

#if !(defined(__cpp_lib_to_chars) && __cpp_lib_to_chars >= 201611L)
#error "this program needs std::to_chars for double"
#endif

namespace {

uint64_t bits_of(double x)
{
    uint64_t b;
    memcpy(&b, &x, sizeof b);
    return b;
}

double value_of(uint64_t b)
{
    double x;
    memcpy(&x, &b, sizeof x);
    return x;
}

// the text of `bits` in a block of exactly the measured size
std::string text_of(uint64_t bits, uint32_t *measured)
{
    const uint32_t n = oem::shortest_f64_len(bits);
    std::unique_ptr<uint8_t[]> buf(new uint8_t[n ? n : 1]);
    const uint8_t *end = oem::emit_shortest_f64(buf.get(), bits);
    *measured = n;
    return std::string((const char *)buf.get(), (size_t)(end - buf.get()));
}

uint64_t parse_bits(const char *s) { return bits_of(strtod(s, nullptr)); }

// digits (no trailing zero, no leading zero) and exponent of the text's value: text = [-] digits * 10^exp10
void digits_of(const std::string &t, std::string *digits, int *exp10)
{
    std::string d;
    int frac = 0;
    bool seen_point = false;
    for (char ch : t) {
        if (ch == '-') continue;
        if (ch == '.') {
            seen_point = true;
            continue;
        }
        d.push_back(ch);
        if (seen_point) ++frac;
    }
    const size_t first = d.find_first_not_of('0');
    d = first == std::string::npos ? "0" : d.substr(first);
    int e = -frac;
    while (d.size() > 1 && d.back() == '0') {
        d.pop_back();
        ++e;
    }
    *digits = d;
    *exp10 = e;
}

// digits * 10^exp10 the way Rust's `{}` places them
std::string positional(bool neg, const std::string &d, int e)
{
    std::string s = neg ? "-" : "";
    const int n = (int)d.size();
    if (e >= 0) return s + d + std::string((size_t)e, '0');
    if (n > -e) return s + d.substr(0, (size_t)(n + e)) + "." + d.substr((size_t)(n + e));
    return s + "0." + std::string((size_t)(-e - n), '0') + d;
}

int fail_at(uint64_t bits, const char *what, const std::string &text)
{
    fprintf(stderr, "0x%016" PRIx64 ": %s (text %s)\n", bits, what, text.c_str());
    return 1;
}

int check_one(uint64_t bits, uint32_t *longest)
{
    uint32_t n = 0;
    const std::string t = text_of(bits, &n);
    if (t.size() != n) return fail_at(bits, "measured length differs from the emitted length", t);
    if (n > *longest) *longest = n;
    if (n > oem::kShortestF64MaxLen) return fail_at(bits, "longer than the header's bound", t);
    if (parse_bits(t.c_str()) != bits) return fail_at(bits, "strtod does not read the text back", t);
    if (t.find('e') != std::string::npos || t.find('E') != std::string::npos) return fail_at(bits, "an exponent", t);
    std::string d;
    int e;
    digits_of(t, &d, &e);
    const bool neg = (bits >> 63) != 0;
    if ((bits << 1) == 0) return t == (neg ? "-0" : "0") ? 0 : fail_at(bits, "zero is `0` / `-0`", t);
    if (d.size() > oem::kShortestF64MaxDigits) return fail_at(bits, "more than 17 significant digits", t);
    if (d.size() > 1) {
        const uint64_t v = strtoull(d.c_str(), nullptr, 10);
        char cand[64];
        for (uint64_t c : {v / 10, v / 10 + 1}) {
            snprintf(cand, sizeof cand, "%s%" PRIu64 "e%d", neg ? "-" : "", c, e + 1);
            if (parse_bits(cand) == bits) return fail_at(bits, (std::string("a shorter decimal reads back the same: ") + cand).c_str(), t);
        }
    }
    {
        char sci[64];
        const auto r = std::to_chars(sci, sci + sizeof sci - 1, value_of(bits), std::chars_format::scientific);
        *r.ptr = 0;
        // [-]d.ddddde[+-]XX
        std::string ds;
        const char *p = sci;
        for (; *p && *p != 'e'; ++p)
            if (*p != '.' && *p != '-') ds.push_back(*p);
        int sci_e = atoi(p + 1) - ((int)ds.size() - 1);
        while (ds.size() > 1 && ds.back() == '0') {
            ds.pop_back();
            ++sci_e;
        }
        if (ds != d || sci_e != e) return fail_at(bits, (std::string("std::to_chars prints ") + sci).c_str(), t);
        if (positional(neg, ds, sci_e) != t) return fail_at(bits, "not std::to_chars' digits in positional form", t);
    }
    return 0;
}

uint64_t splitmix64(uint64_t *s)
{
    uint64_t z = (*s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

std::vector<uint64_t> named_patterns()
{
    std::vector<uint64_t> v;
    auto with_neighbours = [&](uint64_t b) {
        for (uint64_t x : {b - 1, b, b + 1})
            if (x >= 1 && x < 0x7ff0000000000000ull) v.push_back(x);
    };
    for (int e = -1074; e <= 1023; ++e) with_neighbours(bits_of(ldexp(1.0, e)));
    for (int k = -323; k <= 308; ++k) {
        char s[16];
        snprintf(s, sizeof s, "1e%d", k);
        with_neighbours(parse_bits(s));
    }
    v.push_back(1);                                 // 5e-324
    v.push_back(0x000fffffffffffffull);             // the largest subnormal
    v.push_back(0x0010000000000000ull);             // the smallest normal
    v.push_back(bits_of(DBL_MAX));
    for (double x : {9007199254740991.0, 9007199254740992.0, 9007199254740994.0, 0.1 + 0.2, 1e21, 1e22, 1e23, 0.0})
        v.push_back(bits_of(x));
    v.push_back(parse_bits("9007199254740993")); // no f64: the tie goes to 2^53
    // from the test sets of Ryu, Grisu and double-conversion: 17-digit values, values whose shortest form needs the
    // round-to-odd bit, values at the edges of the table
    for (const char *s : {"1.7976931348623157e308", "2.2250738585072014e-308", "4.9406564584124654e-324", "1.8531501765868567e21",
                          "-3.347727380279489e33", "1.9430376160308388e16", "-6.9741824662760956e19", "4.3816050601147837e18",
                          "9.5e-322", "2.98023223876953125e-8", "5.764607523034235e39", "1.152921504606847e40",
                          "2.305843009213694e40", "1.2345678e0", "4.294967294e0", "4.294967295e0", "4.294967296e0",
                          "1.2e1", "1.23e2", "8.41e21", "2.0019999999999998e0", "9.5367431640625e-7", "4.8e-322",
                          "1.8446744073709552e19", "5e-324", "1.7800590868057611e-307", "2.8480945388892175e-306",
                          "2.446494580089078e-296", "4.8929891601781557e-296", "1.8014398509481984e16", "3.6028797018963964e16",
                          "2.900835519859558e-216", "5.801671039719115e-216", "3.196104012172126e-27", "9.007199254740991e15",
                          "1.2345678901234567e0", "0.3", "2.5", "123456789012345680000"})
        v.push_back(parse_bits(s));
    const size_t n = v.size();
    for (size_t i = 0; i < n; ++i) v.push_back(v[i] | 0x8000000000000000ull);
    v.push_back(0x8000000000000000ull);
    return v;
}

int sweep(uint64_t n_random, uint64_t seed)
{
    uint32_t longest = 0;
    uint64_t n = 0;
    for (uint64_t b : named_patterns()) {
        if (check_one(b, &longest)) return 1;
        ++n;
    }
    // the fixed texts of the format
    struct Fixed {
        double x;
        const char *text;
    };
    for (const Fixed &f : {Fixed{1.0, "1"}, Fixed{0.1, "0.1"}, Fixed{1e23, "100000000000000000000000"}, Fixed{-0.0, "-0"},
                           Fixed{0.0, "0"}, Fixed{0.1 + 0.2, "0.30000000000000004"}, Fixed{9007199254740992.0, "9007199254740992"},
                           Fixed{-2.5, "-2.5"}, Fixed{1e21, "1000000000000000000000"}}) {
        uint32_t m = 0;
        const std::string t = text_of(bits_of(f.x), &m);
        if (t != f.text) return fail_at(bits_of(f.x), f.text, t);
    }
    {
        uint32_t m = 0;
        const std::string t = text_of(1, &m);
        if (t != "0." + std::string(323, '0') + "5") return fail_at(1, "5e-324 is `0.`, 323 zeros, `5`", t);
    }
    for (uint64_t i = 0; i < n_random; ++n) {
        const uint64_t b = splitmix64(&seed);
        if ((b & 0x7ff0000000000000ull) == 0x7ff0000000000000ull) continue; // an infinity or a NaN
        if (check_one(b, &longest)) return 1;
        ++i;
    }
    // the bound is attained: a sign, `0.` and 324 fraction digits (the negative of the smallest subnormal)
    uint32_t m = 0;
    const std::string neg = text_of(0x8000000000000001ull, &m);
    if (m != oem::kShortestF64MaxLen || neg.size() != m || longest != oem::kShortestF64MaxLen) {
        fprintf(stderr, "longest text %u, header's bound %u\n", longest, oem::kShortestF64MaxLen);
        return 1;
    }
    printf("checked %" PRIu64 " longest %u bound %u\n", n, longest, oem::kShortestF64MaxLen);
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "--sweep")) return sweep(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10));
    char line[64];
    while (fgets(line, sizeof line, stdin)) {
        char *end = nullptr;
        const unsigned long long b = strtoull(line, &end, 16);
        if (end == line) {
            fprintf(stderr, "bad request: %s", line);
            return 2;
        }
        uint32_t n = 0;
        const std::string t = text_of((uint64_t)b, &n);
        printf("%s %u\n", t.c_str(), n);
    }
    return 0;
}
