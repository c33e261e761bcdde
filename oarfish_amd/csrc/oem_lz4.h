// oem_lz4.h -- the LZ4 frame and block formats as far as `.prob.lz4` needs them (oem_assignment_text_lz4).
//
// Reference: write_function::write_out_prob with `--compressed-probs` (src/util/write_function.rs:243-263, 334-337)
// hands the text to the `lz4` crate's frame encoder.  The formats are the public ones: "LZ4 Frame Format" v1.6.x,
// "LZ4 Block Format", and XXH32 of the xxHash specification.  The functions here are pure (host and device; nothing
// from HIP, so a host compiler builds them and tests/test_lz4_format.py holds them to a decoder written from the
// documents, and to liblz4 where there is one).  As in oem_text_format.h "measure" and "emit" are one family: a
// sequence's bytes are described once (SeqLayout, seq_head_byte, seq_tail_byte); its length, the serial emitter
// below and the cooperative emitter of k_lz4_blocks (oem_lz4.hip) all read that description, so a length can never
// disagree with the bytes written.
//
// The frame this project writes: magic, FLG 0x78 (version 01, independent blocks, block checksums, content size, no
// content checksum, no dictionary id), BD 0x40 (blocks of at most 64 KiB), the content size, HC; the blocks, each
// `size word | payload | XXH32(payload)`; the zero EndMark.  A content checksum is deliberately left out: XXH32 over
// the whole content is one serial chain, while the per-block checksums, which carry the integrity instead, are as
// parallel as the blocks are.
#pragma once

#include <stdint.h>
#include <string.h>

#ifndef OEM_HD
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define OEM_HD __host__ __device__
#else
#define OEM_HD
#endif
#endif

namespace oem {
namespace lz4 {

// -- XXH32 -------------------------------------------------------------------------------------------------------------
constexpr uint32_t kP1 = 2654435761u, kP2 = 2246822519u, kP3 = 3266489917u, kP4 = 668265263u, kP5 = 374761393u;

OEM_HD inline uint32_t rotl32(uint32_t x, uint32_t r) { return (x << r) | (x >> (32u - r)); }

OEM_HD inline uint32_t read_le32(const uint8_t *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// accumulator i (0 .. 3) of a 16-byte stripe before the first stripe
OEM_HD inline uint32_t xxh32_acc_init(uint32_t i, uint32_t seed)
{
    return i == 0 ? seed + kP1 + kP2 : i == 1 ? seed + kP2 : i == 2 ? seed : seed - kP1;
}

OEM_HD inline uint32_t xxh32_round(uint32_t acc, uint32_t in)
{
    acc += in * kP2;
    return rotl32(acc, 13) * kP1;
}

// The accumulators after the n / 16 stripes (unused when n < 16), then the n % 16 bytes at `tail`.
OEM_HD inline uint32_t xxh32_finish(uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, const uint8_t *tail, uint64_t n,
                                    uint32_t seed)
{
    uint32_t h = n >= 16 ? rotl32(v0, 1) + rotl32(v1, 7) + rotl32(v2, 12) + rotl32(v3, 18) : seed + kP5;
    h += (uint32_t)n;
    uint32_t left = (uint32_t)(n & 15u);
    for (; left >= 4; left -= 4, tail += 4) h = rotl32(h + read_le32(tail) * kP3, 17) * kP4;
    for (; left; --left, ++tail) h = rotl32(h + (uint32_t)*tail * kP5, 11) * kP1;
    h ^= h >> 15;
    h *= kP2;
    h ^= h >> 13;
    h *= kP3;
    h ^= h >> 16;
    return h;
}

OEM_HD inline uint32_t xxh32(const uint8_t *p, uint64_t n, uint32_t seed = 0)
{
    uint32_t v[4];
    for (uint32_t i = 0; i < 4; ++i) v[i] = xxh32_acc_init(i, seed);
    const uint64_t stripes = n / 16;
    for (uint64_t s = 0; s < stripes; ++s)
        for (uint32_t i = 0; i < 4; ++i) v[i] = xxh32_round(v[i], read_le32(p + 16 * s + 4 * i));
    return xxh32_finish(v[0], v[1], v[2], v[3], p + 16 * stripes, n, seed);
}

// -- the frame ---------------------------------------------------------------------------------------------------------
constexpr uint32_t kFrameHeaderBytes = 15; // magic 4, FLG, BD, content size 8, HC
constexpr uint32_t kEndMarkBytes = 4;
constexpr uint32_t kBlockMaxBytes = 65536;      // BD 0x40
constexpr uint32_t kBlockRawBit = 0x80000000u;  // of a block's size word: the payload is the content itself
constexpr uint32_t kBlockOverheadBytes = 8;     // size word + block checksum

OEM_HD inline void put_le32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
    p[2] = (uint8_t)(v >> 16);
    p[3] = (uint8_t)(v >> 24);
}

// out[0 .. 15): the frame descriptor of a frame whose content is `content_bytes` long
OEM_HD inline void frame_header(uint8_t *out, uint64_t content_bytes)
{
    put_le32(out, 0x184D2204u);
    out[4] = 0x78;
    out[5] = 0x40;
    for (uint32_t i = 0; i < 8; ++i) out[6 + i] = (uint8_t)(content_bytes >> (8 * i));
    out[14] = (uint8_t)(xxh32(out + 4, 10) >> 8);
}

// -- the block format --------------------------------------------------------------------------------------------------
constexpr uint32_t kMinMatch = 4;
constexpr uint32_t kMatchFreeTail = 12; // no match starts in the last 12 bytes of a block
constexpr uint32_t kLastLiterals = 5;   // the last 5 bytes of a block are literals
constexpr uint32_t kMinMatchBlock = 13; // a shorter block is all literals

// the worst-case size of a compressed block of n bytes
OEM_HD inline uint32_t block_bound(uint32_t n) { return n + n / 255u + 16u; }

// A length is a 4-bit code in the token (the literal length, or the match length - 4) and, from 15 on, extension bytes
// that add up to the rest: (code - 15) / 255 bytes of 255, then one of (code - 15) % 255.
OEM_HD inline uint32_t ext_count(uint32_t code) { return code >= 15u ? 1u + (code - 15u) / 255u : 0u; }

OEM_HD inline uint8_t ext_byte(uint32_t code, uint32_t i)
{
    return i + 1u < ext_count(code) ? (uint8_t)255 : (uint8_t)((code - 15u) % 255u);
}

// Where the parts of a sequence lie.  match_len == 0: the last sequence of a block, literals only (no offset).
struct SeqLayout {
    uint32_t head;  // token + literal-length extension bytes; the literals follow at [head, head + lit_len)
    uint32_t tail;  // offset (2) + match-length extension bytes, at [head + lit_len, total); 0 for the last sequence
    uint32_t total;
};

OEM_HD inline SeqLayout seq_layout(uint32_t lit_len, uint32_t match_len)
{
    SeqLayout l;
    l.head = 1u + ext_count(lit_len);
    l.tail = match_len ? 2u + ext_count(match_len - kMinMatch) : 0u;
    l.total = l.head + lit_len + l.tail;
    return l;
}

// the byte length of a sequence / of the last-literals sequence
OEM_HD inline uint32_t seq_bytes(uint32_t lit_len, uint32_t match_len) { return seq_layout(lit_len, match_len).total; }
OEM_HD inline uint32_t last_literals_bytes(uint32_t lit_len) { return seq_layout(lit_len, 0).total; }

// byte i of the head, i < seq_layout().head
OEM_HD inline uint8_t seq_head_byte(uint32_t lit_len, uint32_t match_len, uint32_t i)
{
    if (i) return ext_byte(lit_len, i - 1u);
    const uint32_t mcode = match_len ? match_len - kMinMatch : 0u;
    return (uint8_t)(((lit_len < 15u ? lit_len : 15u) << 4) | (mcode < 15u ? mcode : 15u));
}

// byte i of the tail, i < seq_layout().tail: the offset, little-endian, then the match-length extension
OEM_HD inline uint8_t seq_tail_byte(uint32_t offset, uint32_t match_len, uint32_t i)
{
    if (i < 2u) return (uint8_t)(offset >> (8u * i));
    return ext_byte(match_len - kMinMatch, i - 2u);
}

// One sequence at p, serially: `lit_len` literals from `lit`, then a match of `match_len` >= 4 bytes `offset` back
// (match_len == 0: the last literals).  Returns the byte after the last, p + seq_bytes(lit_len, match_len).
OEM_HD inline uint8_t *emit_sequence(uint8_t *p, const uint8_t *lit, uint32_t lit_len, uint32_t offset, uint32_t match_len)
{
    const SeqLayout l = seq_layout(lit_len, match_len);
    for (uint32_t i = 0; i < l.head; ++i) p[i] = seq_head_byte(lit_len, match_len, i);
    p += l.head;
    for (uint32_t i = 0; i < lit_len; ++i) p[i] = lit[i];
    p += lit_len;
    for (uint32_t i = 0; i < l.tail; ++i) p[i] = seq_tail_byte(offset, match_len, i);
    return p + l.tail;
}

OEM_HD inline uint8_t *emit_last_literals(uint8_t *p, const uint8_t *lit, uint32_t lit_len)
{
    return emit_sequence(p, lit, lit_len, 0, 0);
}

// the hash of the 4 bytes a match candidate is looked up by: `bits` bits of a multiplicative hash
OEM_HD inline uint32_t hash4(uint32_t v, uint32_t bits) { return (v * 2654435761u) >> (32u - bits); }

} // namespace lz4
} // namespace oem
