// Stand-alone driver of oarfish_amd/csrc/oem_lz4.h for tests/test_lz4_format.py (host compiler, sanitizers on).
// stdin, one request per line (bytes as hex, "-" for none):
//   x <bytes>          -> XXH32 of the bytes, seed 0, hex
//   h <content size>   -> the 15 bytes of the frame descriptor, hex
//   g <bytes>          -> the bytes as ONE compressed block by the serial greedy parser below, over the header's
//                         emitters: "<block, hex> <measured length> <lit:match:offset of every sequence, comma-joined>"
// Every output buffer is exactly the measured size: one byte more is a sanitizer report.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../oarfish_amd/csrc/oem_lz4.h"

namespace lz4 = oem::lz4;

static bool unhex(const std::string &s, std::vector<uint8_t> *out)
{
    out->clear();
    if (s == "-") return true;
    if (s.size() % 2) return false;
    auto nib = [](char c) -> int { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; };
    out->reserve(s.size() / 2);
    for (size_t i = 0; i < s.size(); i += 2) {
        const int a = nib(s[i]), b = nib(s[i + 1]);
        if (a < 0 || b < 0) return false;
        out->push_back((uint8_t)(a * 16 + b));
    }
    return true;
}

static void put_hex(const uint8_t *p, size_t n)
{
    if (!n) fputs("-", stdout);
    for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
}

struct Seq {
    uint32_t lit, match, offset;
};

// Greedy, one position at a time: the last position with the same 4 bytes is the candidate.  The block format's end
// rules as the kernel keeps them: a match starts before the last 12 bytes and ends before the last 5.
static std::vector<Seq> parse(const std::vector<uint8_t> &src)
{
    std::vector<Seq> seqs;
    const uint32_t n = (uint32_t)src.size();
    uint32_t anchor = 0;
    if (n >= lz4::kMinMatchBlock) {
        std::unordered_map<uint32_t, uint32_t> table; // the 4 bytes -> their last position
        const uint32_t match_limit = n - lz4::kMatchFreeTail, match_end = n - lz4::kLastLiterals;
        auto key = [&](uint32_t p) { return lz4::read_le32(src.data() + p); };
        uint32_t p = 0;
        while (p < match_limit) {
            const uint32_t h = key(p);
            const auto it = table.find(h);
            const int64_t c = it == table.end() ? -1 : (int64_t)it->second;
            table[h] = p;
            if (c < 0 || p - c > 65535) {
                ++p;
                continue;
            }
            uint32_t len = lz4::kMinMatch;
            while (p + len < match_end && src[p + len] == src[(size_t)c + len]) ++len;
            seqs.push_back({p - anchor, len, (uint32_t)(p - c)});
            for (uint32_t q = p + 1; q < p + len && q < match_limit; ++q) table[key(q)] = q;
            p += len;
            anchor = p;
        }
    }
    seqs.push_back({n - anchor, 0, 0});
    return seqs;
}

int main()
{
    std::string line;
    std::vector<uint8_t> data;
    while (std::getline(std::cin, line)) {
        if (line.size() < 3 || line[1] != ' ') {
            fprintf(stderr, "bad request\n");
            return 2;
        }
        const std::string arg = line.substr(2);
        if (line[0] == 'x') {
            if (!unhex(arg, &data)) return 2;
            std::vector<uint8_t> exact(data); // (its own allocation of exactly n bytes: a read past the end is reported)
            printf("%08" PRIx32 "\n", lz4::xxh32(exact.data(), exact.size()));
        } else if (line[0] == 'h') {
            std::vector<uint8_t> hdr(lz4::kFrameHeaderBytes);
            lz4::frame_header(hdr.data(), strtoull(arg.c_str(), nullptr, 10));
            put_hex(hdr.data(), hdr.size());
            printf("\n");
        } else if (line[0] == 'g') {
            if (!unhex(arg, &data)) return 2;
            const std::vector<Seq> seqs = parse(data);
            uint64_t measured = 0;
            for (const Seq &s : seqs) measured += lz4::seq_bytes(s.lit, s.match);
            if (seqs.back().match != 0 || lz4::last_literals_bytes(seqs.back().lit) != lz4::seq_bytes(seqs.back().lit, 0)) return 3;
            if (measured > lz4::block_bound((uint32_t)data.size())) {
                fprintf(stderr, "%" PRIu64 " bytes measured, above the bound\n", measured);
                return 3;
            }
            std::vector<uint8_t> out(measured);
            uint8_t *p = out.data();
            uint32_t at = 0;
            for (const Seq &s : seqs) {
                uint8_t *const end = s.match ? lz4::emit_sequence(p, data.data() + at, s.lit, s.offset, s.match)
                                             : lz4::emit_last_literals(p, data.data() + at, s.lit);
                if (end != p + lz4::seq_bytes(s.lit, s.match)) {
                    fprintf(stderr, "a sequence's emitted length differs from its measured length\n");
                    return 3;
                }
                p = end;
                at += s.lit + s.match;
            }
            if (p != out.data() + measured || at != data.size()) return 3;
            put_hex(out.data(), out.size());
            printf(" %" PRIu64 " ", measured);
            for (size_t i = 0; i < seqs.size(); ++i) printf("%s%u:%u:%u", i ? "," : "", seqs[i].lit, seqs[i].match, seqs[i].offset);
            printf("\n");
        } else {
            fprintf(stderr, "bad request\n");
            return 2;
        }
    }
    return 0;
}
