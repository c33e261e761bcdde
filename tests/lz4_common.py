"""What the LZ4 tests share, written from the format documents ("LZ4 Frame Format", "LZ4 Block Format", the xxHash
specification) and independent of oarfish_amd/csrc/oem_lz4.h: XXH32, a strict frame and block decoder, and a ctypes
handle on the system's liblz4 where there is one."""
import ctypes as C
import struct

M32 = 0xFFFFFFFF
P1, P2, P3, P4, P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def xxh32(data, seed=0):
    data = bytes(data)
    n = len(data)
    at = 0
    if n >= 16:
        stripes = n // 16
        words = struct.unpack_from(f"<{4 * stripes}I", data)
        acc = []
        for i, v in enumerate(((seed + P1 + P2) & M32, (seed + P2) & M32, seed & M32, (seed - P1) & M32)):
            for w in words[i::4]:
                v = (v + w * P2) & M32
                v = (((v << 13) | (v >> 19)) & M32) * P1 & M32
            acc.append(v)
        h = (_rotl(acc[0], 1) + _rotl(acc[1], 7) + _rotl(acc[2], 12) + _rotl(acc[3], 18)) & M32
        at = 16 * stripes
    else:
        h = (seed + P5) & M32
    h = (h + n) & M32
    while at + 4 <= n:
        h = (h + struct.unpack_from("<I", data, at)[0] * P3) & M32
        h = _rotl(h, 17) * P4 & M32
        at += 4
    while at < n:
        h = (h + data[at] * P5) & M32
        h = _rotl(h, 11) * P1 & M32
        at += 1
    h ^= h >> 15
    h = h * P2 & M32
    h ^= h >> 13
    h = h * P3 & M32
    h ^= h >> 16
    return h


MAGIC = b"\x04\x22\x4d\x18"
HEADER_BYTES = 15
BLOCK_MAX = 65536


def frame_header(content_size):
    """The descriptor this project writes: FLG 0x78, BD 0x40, the content size, HC."""
    desc = bytes([0x78, 0x40]) + struct.pack("<Q", content_size)
    return MAGIC + desc + bytes([(xxh32(desc) >> 8) & 0xFF])


class FormatError(ValueError):
    pass


def decode_block(payload, max_out=None):
    """One compressed block -> its bytes (see block_sequences for its parse)."""
    return _decode_block(payload, max_out)[0]


def block_sequences(payload):
    """The (literal length, match length, offset) of every sequence of a compressed block; the last is (n, 0, 0)."""
    return _decode_block(payload, None)[1]


def _decode_block(payload, max_out):
    """One compressed block -> (its bytes, its sequences), refusing what the block format forbids: offset 0, an offset beyond the
    block's output, a match that starts in the last 12 bytes or reaches into the last 5, a final sequence with a
    match, input that ends inside a sequence."""
    src = bytes(payload)
    n = len(src)
    out = bytearray()
    match_starts = []
    seqs = []
    at = 0
    if n == 0:
        raise FormatError("an empty compressed block")
    while True:
        token = src[at]
        at += 1
        lit = token >> 4
        if lit == 15:
            while True:
                if at >= n:
                    raise FormatError("input ends inside a literal length")
                b = src[at]
                at += 1
                lit += b
                if b != 255:
                    break
        if at + lit > n:
            raise FormatError("literals run past the block")
        out += src[at:at + lit]
        at += lit
        if at == n:
            if token & 15:
                raise FormatError("the final sequence carries a match length")
            seqs.append((lit, 0, 0))
            break
        if at + 2 > n:
            raise FormatError("input ends inside an offset")
        offset = src[at] | (src[at + 1] << 8)
        at += 2
        if offset == 0:
            raise FormatError("offset 0")
        if offset > len(out):
            raise FormatError("offset beyond the block's output")
        ml = token & 15
        if ml == 15:
            while True:
                if at >= n:
                    raise FormatError("input ends inside a match length")
                b = src[at]
                at += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        if at >= n:
            raise FormatError("the final sequence carries a match")
        match_starts.append((len(out), ml))
        seqs.append((lit, ml, offset))
        start = len(out) - offset
        if offset >= ml:
            out += out[start:start + ml]
        else:                                   # the copy overlaps what it writes: the pattern repeats
            pat = bytes(out[start:])
            out += (pat * (ml // offset + 1))[:ml]
        if max_out is not None and len(out) > max_out:
            raise FormatError("the block decodes to more than the block maximum")
    total = len(out)
    for start, ml in match_starts:
        if start + 12 > total:
            raise FormatError(f"a match starts {total - start} bytes before the end of the block")
        if start + ml + 5 > total:
            raise FormatError("a match reaches into the last 5 bytes")
    if match_starts and total < 13:
        raise FormatError("a match in a block shorter than 13 bytes")
    return bytes(out), seqs


class Frame:
    def __init__(self):
        self.content = b""
        self.content_size = None
        self.blocks = []          # (stored size, raw?, decoded length)
        self.payloads = []        # the blocks' payloads as stored

    @property
    def n_blocks(self):
        return len(self.blocks)

    @property
    def raw_blocks(self):
        return sum(1 for b in self.blocks if b[1])


def decode_frame(frame, strict_descriptor=True):
    """A whole frame -> Frame.  Verifies magic, HC, every block checksum that is present, the content size and
    checksum where present, the EndMark and that nothing follows it.  strict_descriptor: the descriptor must be the
    one this project writes (FLG 0x78, BD 0x40)."""
    f = bytes(frame)
    if f[:4] != MAGIC:
        raise FormatError("magic")
    flg, bd = f[4], f[5]
    if flg >> 6 != 1:
        raise FormatError("version")
    if strict_descriptor and (flg, bd) != (0x78, 0x40):
        raise FormatError(f"descriptor FLG {flg:#x} BD {bd:#x}")
    independent, block_sum, has_size, content_sum, dict_id = flg & 0x20, flg & 0x10, flg & 0x08, flg & 0x04, flg & 0x01
    if flg & 0x02 or bd & 0x8F:
        raise FormatError("reserved bits")
    block_max = {4: 1 << 16, 5: 1 << 18, 6: 1 << 20, 7: 1 << 22}.get(bd >> 4)
    if block_max is None:
        raise FormatError("block maximum")
    at = 6
    out = Frame()
    if has_size:
        out.content_size = struct.unpack_from("<Q", f, at)[0]
        at += 8
    if dict_id:
        at += 4
    if f[at] != (xxh32(f[4:at]) >> 8) & 0xFF:
        raise FormatError("HC")
    at += 1
    parts = []
    history = b""
    while True:
        if at + 4 > len(f):
            raise FormatError("the frame ends without an EndMark")
        word = struct.unpack_from("<I", f, at)[0]
        at += 4
        if word == 0:
            break
        raw, size = word >> 31, word & 0x7FFFFFFF
        if size > block_max:
            raise FormatError("a block larger than the block maximum")
        if at + size + (4 if block_sum else 0) > len(f):
            raise FormatError("a block runs past the frame")
        payload = f[at:at + size]
        at += size
        if block_sum:
            if struct.unpack_from("<I", f, at)[0] != xxh32(payload):
                raise FormatError(f"checksum of block {len(parts)}")
            at += 4
        if raw:
            data = payload
        elif independent:
            data = decode_block(payload, block_max)
        else:
            raise FormatError("linked blocks: not decoded here")
        if len(data) > block_max:
            raise FormatError("a block decodes to more than the block maximum")
        out.blocks.append((size, bool(raw), len(data)))
        out.payloads.append(payload)
        parts.append(data)
    out.content = b"".join(parts)
    if content_sum:
        if struct.unpack_from("<I", f, at)[0] != xxh32(out.content):
            raise FormatError("content checksum")
        at += 4
    if at != len(f):
        raise FormatError("bytes after the frame")
    if out.content_size is not None and out.content_size != len(out.content):
        raise FormatError(f"content size {out.content_size} != {len(out.content)} decoded")
    return out


_system = False


def system_lz4():
    """liblz4.so.1 through ctypes, or None."""
    global _system
    if _system is False:
        try:
            L = C.CDLL("liblz4.so.1")
            L.LZ4F_isError.argtypes = [C.c_size_t]
            L.LZ4F_createDecompressionContext.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
            L.LZ4F_createDecompressionContext.restype = C.c_size_t
            L.LZ4F_freeDecompressionContext.argtypes = [C.c_void_p]
            L.LZ4F_freeDecompressionContext.restype = C.c_size_t
            L.LZ4F_decompress.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p,
                                          C.POINTER(C.c_size_t), C.c_void_p]
            L.LZ4F_decompress.restype = C.c_size_t
            L.LZ4F_compressFrameBound.argtypes = [C.c_size_t, C.c_void_p]
            L.LZ4F_compressFrameBound.restype = C.c_size_t
            L.LZ4F_compressFrame.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
            L.LZ4F_compressFrame.restype = C.c_size_t
            L.LZ4_decompress_safe.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
            L.LZ4_decompress_safe.restype = C.c_int
            L.LZ4_compress_default.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
            L.LZ4_compress_default.restype = C.c_int
            L.LZ4_compressBound.argtypes = [C.c_int]
            L.LZ4_compressBound.restype = C.c_int
            _system = L
        except (OSError, AttributeError):
            _system = None
    return _system


def system_decode_frame(frame, expect_len):
    """LZ4F_decompress of a whole frame (it verifies the checksums the frame carries)."""
    L = system_lz4()
    ctx = C.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createDecompressionContext(C.byref(ctx), 100))
    try:
        src = C.create_string_buffer(bytes(frame), len(frame))
        dst = C.create_string_buffer(max(expect_len, 1) + 64)
        s_at, d_at, hint = 0, 0, 1
        while s_at < len(frame):
            s_n, d_n = C.c_size_t(len(frame) - s_at), C.c_size_t(len(dst) - d_at)
            hint = L.LZ4F_decompress(ctx, C.byref(dst, d_at), C.byref(d_n), C.byref(src, s_at), C.byref(s_n), None)
            if L.LZ4F_isError(hint):
                raise FormatError(f"LZ4F_decompress: error {-hint & M32}")
            s_at += s_n.value
            d_at += d_n.value
            if hint == 0 or (s_n.value == 0 and d_n.value == 0):
                break
        if hint != 0:
            raise FormatError("LZ4F_decompress: the frame is incomplete")
        if s_at != len(frame):
            raise FormatError("LZ4F_decompress: bytes after the frame")
        return dst.raw[:d_at]
    finally:
        L.LZ4F_freeDecompressionContext(ctx)


def system_decode_block(payload, n_out):
    L = system_lz4()
    dst = C.create_string_buffer(max(n_out, 1))
    got = L.LZ4_decompress_safe(bytes(payload), dst, len(payload), n_out)
    if got < 0:
        raise FormatError(f"LZ4_decompress_safe: {got}")
    return dst.raw[:got]


class FramePrefs(C.Structure):
    """LZ4F_preferences_t of liblz4 1.9.x."""
    _fields_ = [("blockSizeID", C.c_int), ("blockMode", C.c_int), ("contentChecksumFlag", C.c_int),
                ("frameType", C.c_int), ("contentSize", C.c_ulonglong), ("dictID", C.c_uint),
                ("blockChecksumFlag", C.c_int), ("compressionLevel", C.c_int), ("autoFlush", C.c_uint),
                ("favorDecSpeed", C.c_uint), ("reserved", C.c_uint * 3)]


def system_compress_frame(data, level=0, independent=True, block_sum=True, content_sum=False):
    L = system_lz4()
    p = FramePrefs()
    p.blockSizeID = 4                            # 64 KiB
    p.blockMode = 1 if independent else 0
    p.contentChecksumFlag = 1 if content_sum else 0
    p.contentSize = len(data)
    p.blockChecksumFlag = 1 if block_sum else 0
    p.compressionLevel = level
    cap = L.LZ4F_compressFrameBound(len(data), C.byref(p))
    dst = C.create_string_buffer(cap)
    n = L.LZ4F_compressFrame(dst, cap, bytes(data), len(data), C.byref(p))
    assert not L.LZ4F_isError(n)
    return dst.raw[:n]


def decode_everywhere(frame, strict_descriptor=True):
    """The Python decoder's Frame; and liblz4's verdict on the same bytes, where the library exists."""
    out = decode_frame(frame, strict_descriptor)
    if system_lz4() is not None:
        assert system_decode_frame(frame, len(out.content)) == out.content
    return out
