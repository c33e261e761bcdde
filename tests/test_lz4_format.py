"""CPU test of the LZ4 frame and block primitives (oarfish_amd/csrc/oem_lz4.h): the header's pure functions -- the ones
k_lz4_blocks of oem_lz4.hip calls -- are compiled into a stand-alone host program with the address and
undefined-behaviour sanitizers on, and held to a decoder and an XXH32 written from the format documents
(tests/lz4_common.py), and to the system's liblz4 where there is one.  The program gives every emitter a buffer of
exactly the measured size, so one byte more is a sanitizer report."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import lz4_common as lz

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "lz4_format_main.cpp")
EXE = os.path.join(HERE, "native", "lz4_format_main")
HDR = os.path.join(HERE, "..", "oarfish_amd", "csrc", "oem_lz4.h")


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-o", EXE, SRC])
    return EXE


def run(exe, requests):
    r = subprocess.run([exe], input="".join(requests), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[-1] == "" and len(out) == len(requests) + 1
    return out[:-1]


def hexed(b):
    return bytes(b).hex() or "-"


def test_xxh32(exe):
    assert lz.xxh32(b"") == 0x02CC5D05
    assert run(exe, ["x -\n"]) == ["02cc5d05"]
    # the specification's own vectors pin the Python side (seed 0; the 0x9E3779B1 sequence of the xxHash sanity test
    # is not reproduced here: these two come from the algorithm's description and every implementation agrees on them)
    assert lz.xxh32(b"a") == 0x550D7456 and lz.xxh32(b"abc") == 0x32D153FF
    rng = np.random.default_rng(32)
    lengths = list(range(65)) + [65535, 65536] + [int(x) for x in rng.integers(0, 4096, size=1000)]
    datas = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in lengths]
    got = run(exe, [f"x {hexed(d)}\n" for d in datas])
    for d, g in zip(datas, got):
        assert int(g, 16) == lz.xxh32(d), len(d)


def test_descriptor(exe):
    sizes = (0, 1, 2 ** 32 + 5)
    got = run(exe, [f"h {n}\n" for n in sizes])
    for n, g in zip(sizes, got):
        hdr = bytes.fromhex(g)
        assert hdr == lz.frame_header(n) and len(hdr) == 15
        assert hdr[:6] == b"\x04\x22\x4d\x18\x78\x40" and struct.unpack_from("<Q", hdr, 6)[0] == n
        assert hdr[14] == (lz.xxh32(hdr[4:14]) >> 8) & 0xFF
    empty = bytes.fromhex(got[0]) + b"\0\0\0\0"
    assert lz.decode_frame(empty).content == b""
    if lz.system_lz4() is not None:
        assert lz.system_decode_frame(empty, 0) == b""


def random_without_repeats(rng, n):
    """n random bytes among which no 4 consecutive ones occur twice: nothing for a parser to match."""
    while True:
        a = rng.integers(0, 256, size=n, dtype=np.uint8)
        if n < 5:
            return a.tobytes()
        grams = np.lib.stride_tricks.sliding_window_view(a, 4).astype(np.uint32) @ np.array([1, 1 << 8, 1 << 16, 1 << 24], dtype=np.uint32)
        if len(np.unique(grams)) == len(grams):
            return a.tobytes()


def one_match_source(rng, lit_len, match_len, offset):
    """lit_len random bytes, then match_len bytes that repeat what lies `offset` back, then a tail the match cannot run
    into."""
    head = random_without_repeats(rng, lit_len)
    assert offset <= len(head)
    out = bytearray(head)
    for _ in range(match_len):
        out.append(out[-offset])
    stop = (out[-offset] + 1) & 0xFF                      # the byte that ends the match
    return bytes(out) + bytes([stop]) + rng.integers(0, 256, size=15, dtype=np.uint8).tobytes()


LIT_LENS = (14, 15, 16, 269, 270, 271, 65_000)
MATCH_LENS = (4, 18, 19, 20, 273, 274, 275, 65_000)
OFFSETS = (1, 2, 3, 4, 65_535)


def check_blocks(exe, sources, want_first):
    got = run(exe, [f"g {hexed(s)}\n" for s in sources])
    for src, line, want in zip(sources, got, want_first):
        block_hex, measured, parse = line.split(" ")
        block = bytes.fromhex(block_hex)
        seqs = [tuple(int(v) for v in s.split(":")) for s in parse.split(",")]
        assert len(block) == int(measured)
        if want is not None:
            assert want in seqs, (want, seqs[:4])
        assert seqs[-1][1:] == (0, 0) and (len(seqs) == 1 or seqs[-1][0] >= 5)
        assert lz.decode_block(block) == src, want
        if lz.system_lz4() is not None:
            assert lz.system_decode_block(block, len(src)) == src, want


def test_sequences_decode_to_their_source(exe):
    rng = np.random.default_rng(4)
    sources, want = [], []
    for lit in LIT_LENS:                                  # each literal length, against a plain match
        sources.append(one_match_source(rng, lit, 20, 7))
        want.append((lit, 20, 7))
    for ml in MATCH_LENS:                                 # each match length, non-overlapping and overlapping
        for off in (300, 3) if ml < 65_000 else (65_000, 3):
            sources.append(one_match_source(rng, max(off, 40), ml, off))
            want.append((max(off, 40), ml, off))
    for off in OFFSETS:                                   # each offset (1 .. 3: the source overlaps itself)
        for ml in (4, 19, 275):
            sources.append(one_match_source(rng, max(off, 16), ml, off))
            want.append((max(off, 16), ml, off))
    # a literal length of 0: a second match right behind the first
    a = rng.integers(0, 256, size=60, dtype=np.uint8).tobytes()
    sources.append(a + a[0:10] + a[30:45] + rng.integers(0, 256, size=16, dtype=np.uint8).tobytes())
    want.append((0, 15, 40))
    # no match at all, and blocks too short for one
    sources.append(random_without_repeats(rng, 65_000))
    want.append((65_000, 0, 0))
    for n in (0, 1, 12):
        sources.append(b"\0" * n)
        want.append((n, 0, 0))
    sources += [b"\0" * 13, b"\0" * 14]                   # the shortest block with a match has 14 bytes
    want += [(13, 0, 0), (1, 8, 1)]
    check_blocks(exe, sources, want)


def test_end_of_block_rules(exe):
    """A repeat that a greedy match would carry into the last 5 bytes stops before them, and one that would start in the
    last 12 bytes stays literal."""
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, size=100, dtype=np.uint8).tobytes()
    into_tail = a + a[:50]                                # the repeat runs to the very end
    late = a + rng.integers(0, 256, size=30, dtype=np.uint8).tobytes() + a[:11]   # starts 11 before the end
    got = run(exe, [f"g {hexed(s)}\n" for s in (into_tail, late)])
    seqs = [[tuple(int(v) for v in s.split(":")) for s in g.split(" ")[2].split(",")] for g in got]
    assert seqs[0] == [(100, 45, 100), (5, 0, 0)]
    assert seqs[1] == [(141, 0, 0)]
    check_blocks(exe, [into_tail, late], [None, None])


def test_decoder_refuses_format_violations():
    lit = bytes(range(20))
    with pytest.raises(lz.FormatError, match="offset 0"):
        lz.decode_block(bytes([0xF0, 5]) + lit + b"\x00\x00" + bytes([0xC0]) + bytes(12))
    with pytest.raises(lz.FormatError, match="beyond"):
        lz.decode_block(bytes([0xF0, 5]) + lit + b"\x15\x00" + bytes([0xC0]) + bytes(12))
    with pytest.raises(lz.FormatError, match="before the end"):
        lz.decode_block(bytes([0xF0, 5]) + lit + b"\x01\x00" + bytes([0x70]) + bytes(7))     # starts 11 before the end
    with pytest.raises(lz.FormatError, match="final sequence"):
        lz.decode_block(bytes([0xF0, 5]) + lit + b"\x01\x00")
    good = bytes([0xF0, 5]) + lit + b"\x01\x00" + bytes([0x80]) + bytes(8)                  # starts 12 before the end
    assert lz.decode_block(good) == lit + bytes([19]) * 4 + bytes(8)
    frame = lz.frame_header(len(lit) + 12) + struct.pack("<I", len(good)) + good + struct.pack("<I", lz.xxh32(good)) + bytes(4)
    assert lz.decode_everywhere(frame).content == lit + bytes([19]) * 4 + bytes(8)
    bad_sum = bytearray(frame)
    bad_sum[-5] ^= 1
    with pytest.raises(lz.FormatError, match="checksum"):
        lz.decode_frame(bad_sum)
    bad_hc = bytearray(frame)
    bad_hc[14] ^= 1
    with pytest.raises(lz.FormatError, match="HC"):
        lz.decode_frame(bad_hc)
    with pytest.raises(lz.FormatError, match="content size"):
        lz.decode_frame(lz.frame_header(3) + frame[15:])


def test_python_decoder_agrees_with_liblz4():
    """Pins the helper, not the product: frames liblz4 itself makes, from random and from repetitive data."""
    if lz.system_lz4() is None:
        pytest.skip("no system liblz4")
    rng = np.random.default_rng(6)
    random = rng.integers(0, 256, size=150_000, dtype=np.uint8).tobytes()
    text = b"".join(b"read/%x\t2\t%d\t%d\t0.%06d\t0.%06d\n" % (i, i % 977, i % 31, i * 7919 % 10 ** 6, i * 104729 % 10 ** 6)
                    for i in range(6000))
    for data in (random, text, b"\0" * 200_000, b"", b"x"):
        for level in (0, 4):
            frame = lz.system_compress_frame(data, level=level, content_sum=(level == 4))
            got = lz.decode_frame(frame, strict_descriptor=False)
            assert got.content == data and lz.system_decode_frame(frame, len(data)) == data
            assert got.n_blocks == -(-len(data) // 65536)
    assert lz.decode_frame(lz.system_compress_frame(random)).raw_blocks == 3
