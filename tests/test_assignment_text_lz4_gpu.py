"""GPU tests of oem_assignment_text_lz4: the `.prob.lz4` file as one LZ4 frame compressed on the device.

Every frame is decoded by the strict Python decoder of tests/lz4_common.py (written from the format documents: it
verifies HC and every block checksum and refuses what the block format forbids) and, where the system has a liblz4, by
LZ4F_decompress as well.  The crafted inputs go through the test-only library's oem_test_lz4_frame, which runs caller
bytes through the path the product compresses a chunk with; the store tests hold the frame's content to
`prefix + assignment_text(...).text`, which tests/test_assignment_text_gpu.py holds to the host writer."""
import ctypes as C

import numpy as np
import pytest

from oarfish_amd import _lib, synth, writers
from oarfish_amd.types import DeviceStore, InMemoryAlignmentStore
from tests import lz4_common as lz

pytestmark = pytest.mark.gpu

BLOCK = 65536
LENGTHS = (0, 1, 4, 5, 11, 12, 13, 14, 63, 64, 65, 65_535, 65_536, 65_537, 3 * 65_536 + 7)
PERIODS = (1, 2, 3, 4, 5, 63, 64, 65)
BLOCK_BYTES = (BLOCK, 1024, 13)


def device_frame(data: bytes) -> bytes:
    """oem_test_lz4_frame (blocks of OEM_LZ4_BLOCK_BYTES, read from the environment by the test-only library)."""
    L = _lib.testing_lib()
    src = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, dtype=np.uint8)
    n_blocks = -(-len(data) // 13)
    out = np.zeros(len(data) + 8 * n_blocks + 19, dtype=np.uint8)          # the bound at the smallest block length
    n = C.c_uint64(0)
    _lib.check(L.oem_test_lz4_frame(src.ctypes.data if data else None, len(data), out.ctypes.data, len(out), C.byref(n)))
    return out[:n.value].tobytes()


def decoded(data: bytes, block_bytes: int):
    frame = device_frame(data)
    f = lz.decode_everywhere(frame)
    assert f.content == data
    assert f.n_blocks == -(-len(data) // block_bytes)
    assert all(b[2] == block_bytes for b in f.blocks[:-1]) and (not f.blocks or 0 < f.blocks[-1][2] <= block_bytes)
    return frame, f


def hash4(gram: bytes) -> int:
    """The slot of 4 bytes in the kernel's table (oem_lz4.h hash4, 12 bits).  Used only to BUILD inputs whose greedy
    parse is known in advance (no literal evicts the candidate a planted repeat needs); never to judge an output."""
    return (int.from_bytes(gram, "little") * 2654435761 & 0xFFFFFFFF) >> 20


def literals_clear_of(rng, n, before: bytes, after: bytes, keep: bytes, first_not=()):
    """n random bytes such that no 4 bytes of before[-3:] + them + after[:3] repeat or fall into the slot of `keep`,
    and the first of them is none of `first_not` (the bytes that would carry the match before them further)."""
    slot = hash4(keep)
    while True:
        r = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        s = before[-3:] + r + after[:3]
        grams = [s[i:i + 4] for i in range(len(s) - 3)]
        if len(set(grams)) == len(grams) and all(hash4(g) != slot for g in grams) and r[0] not in first_not:
            return r


def base_text(rng, n):
    """n random bytes without a repeat whose first 4 keep their table slot to themselves: a later repeat of the
    beginning finds position 0 (or the last repeat) as its candidate."""
    while True:
        a = literals_clear_of(rng, n, b"", b"", b"\0\0\0\0")
        if not any(hash4(a[i:i + 4]) == hash4(a[:4]) for i in range(1, n - 3)):
            return a


@pytest.fixture(params=BLOCK_BYTES)
def block_bytes(request, monkeypatch):
    monkeypatch.setenv("OEM_LZ4_BLOCK_BYTES", str(request.param))
    return request.param


def test_zero_bytes(block_bytes):
    """All-zero blocks: one literal, then one maximal match at offset 1 up to the last 5 bytes."""
    for n in LENGTHS:
        frame, f = decoded(b"\0" * n, block_bytes)
        for (size, raw, length), payload in zip(f.blocks, f.payloads):
            if length >= 14:
                assert not raw and lz.block_sequences(payload) == [(1, length - 6, 1), (5, 0, 0)], (n, length)
            else:
                assert raw and size == length                 # all literals: one byte more than the content
        if block_bytes == BLOCK and n >= BLOCK:
            # 65 530 = 4 + 15 + 255 * 256 + 231: the token, 256 bytes of 255 and one of 231 -> 257 extension bytes
            assert f.blocks[0][0] == 1 + 1 + 2 + 257 + 6


def test_periodic_patterns(block_bytes):
    rng = np.random.default_rng(12)
    for p in PERIODS:
        unit = rng.integers(0, 256, size=p, dtype=np.uint8).tobytes() if p > 1 else b"\x5a"
        for n in LENGTHS:
            data = (unit * (n // p + 1))[:n]
            frame, f = decoded(data, block_bytes)
            if block_bytes == BLOCK and n >= 65_535:          # a period and one long match per full block
                assert not any(b[1] for b in f.blocks if b[2] == BLOCK) and len(frame) < n // 10, (p, n, len(frame))


def test_random_bytes_are_stored_raw(block_bytes):
    rng = np.random.default_rng(13)
    for n in LENGTHS:
        data = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        frame, f = decoded(data, block_bytes)
        assert f.raw_blocks == f.n_blocks
        assert len(frame) == n + 8 * f.n_blocks + 19


LIT_RUNS = (14, 15, 16, 269, 270, 271)


def test_literal_runs_before_a_repeat(block_bytes):
    """Literal runs around the length code's extension boundaries, each followed by a repeat of earlier text."""
    rng = np.random.default_rng(14)
    base = base_text(rng, 80)                                 # (80: its first repeat lies in the second window)
    data = base + base[:20]
    stops = {base[20]}                                        # each run starts with a byte that ends the match before it
    for run in LIT_RUNS + (16,):
        lit = literals_clear_of(rng, run, data, base, base[:4], stops)
        stops.add(lit[0])
        data += lit + (base[:20] if len(stops) <= len(LIT_RUNS) + 1 else b"")
    frame, f = decoded(data, block_bytes)
    if block_bytes == BLOCK:
        seqs = lz.block_sequences(f.payloads[0])
        assert [s[:2] for s in seqs] == [(80, 20)] + [(run, 20) for run in LIT_RUNS] + [(16, 0)], seqs


def test_end_of_block_rules(block_bytes):
    """A repeat whose greedy match would run into the last 5 bytes stops before them; a repeat that would start within
    the last 12 bytes stays literal."""
    rng = np.random.default_rng(15)
    a = base_text(rng, 100)
    into_tail = a + a[:50]
    late = a + a[:40] + literals_clear_of(rng, 30, a, a[50:61], a[:4], {a[40]}) + a[50:61]
    _, f1 = decoded(into_tail, block_bytes)
    _, f2 = decoded(late, block_bytes)
    if block_bytes == BLOCK:
        assert lz.block_sequences(f1.payloads[0]) == [(100, 45, 100), (5, 0, 0)]
        assert lz.block_sequences(f2.payloads[0]) == [(100, 40, 100), (41, 0, 0)]


def test_the_frame_is_a_function_of_the_input(monkeypatch):
    """64 blocks, twice: table slots that several lanes of a window write are resolved by rule, not by the hardware."""
    monkeypatch.setenv("OEM_LZ4_BLOCK_BYTES", "4096")
    rng = np.random.default_rng(16)
    words = [rng.integers(97, 123, size=int(k), dtype=np.uint8).tobytes() for k in rng.integers(2, 9, size=300)]
    data = b" ".join(words[int(i)] for i in rng.integers(0, 300, size=60_000))[:64 * 4096]
    assert len(data) == 64 * 4096
    first = device_frame(data)
    f = lz.decode_everywhere(first)
    assert f.content == data and f.n_blocks == 64 and f.raw_blocks == 0 and len(first) < len(data)
    assert device_frame(data) == first


# -- through the store -------------------------------------------------------------------------------------------------
N_READS, N_TXPS = 70_000, 3_000


class Case:
    def __init__(self, coverage):
        self.st = synth.make_store(N_READS, N_TXPS, 4.0, seed=411 + coverage, coverage=bool(coverage))
        self.names = [f"read/{i:x}" + ("#" * (i % 7)) for i in range(N_READS)]
        with self.device() as d:
            self.counts, _ = d.em_run(None, 120, 1e-3, 50)
        self.prefix = f"{N_TXPS}\t{N_READS}\n".encode() + "".join(f"T{i}\n" for i in range(N_TXPS)).encode()
        self.plain = {}

    def device(self):
        st = self.st
        return DeviceStore(st.row_ptr, st.tid, st.as_prob, st.cov_prob, st.n_txps)

    def text(self, thresh):
        """The uncompressed call's result: computed once per threshold, shared, left unchanged."""
        if thresh not in self.plain:
            with self.device() as d:
                self.plain[thresh] = d.assignment_text(self.counts, thresh, self.names)
        return self.plain[thresh]


_cases = {}


@pytest.fixture(scope="module", params=[0, 1], ids=["plain", "coverage"])
def case(request):
    if request.param not in _cases:
        _cases[request.param] = Case(request.param)
    return _cases[request.param]


def check_result(res, want, prefix):
    f = lz.decode_everywhere(res.text.tobytes())
    body = want.text.tobytes()
    assert f.content == prefix + body
    assert np.array_equal(res.line_off, want.line_off) and np.array_equal(res.kept, want.kept)
    assert res.content_bytes == len(prefix) + len(body) == f.content_size
    assert res.n_blocks == f.n_blocks and res.raw_blocks == f.raw_blocks
    return f


@pytest.mark.parametrize("thresh", (1e-6, 0.2))
def test_frame_decodes_to_prefix_and_text(case, thresh):
    want = case.text(thresh)
    with case.device() as d:
        res = d.assignment_text_lz4(case.counts, thresh, case.names, prefix=case.prefix)
    f = check_result(res, want, case.prefix)
    assert f.n_blocks == -(-res.content_bytes // BLOCK) and all(b[2] == BLOCK for b in f.blocks[:-1])
    assert res.raw_blocks == 0 and len(res.text) < res.content_bytes
    print(f"frame / content = {len(res.text) / res.content_bytes:.4f}, worst block {max(b[0] / b[2] for b in f.blocks):.4f}")


def test_chunks(case, monkeypatch):
    """A text buffer small enough for many chunks: each chunk ends in a short block, and the prefix -- longer than one
    chunk -- grows the first chunk's buffer."""
    thresh = 1e-6
    want = case.text(thresh)
    buf = 1 << 18
    prefix = case.prefix * (buf // len(case.prefix) + 2)
    assert len(want.text) > 5 * buf and len(prefix) > buf
    monkeypatch.setenv("OEM_TEXT_BUF_BYTES", str(buf))
    monkeypatch.setenv("OEM_TEXT_GRID_BLOCKS", "16")
    with _lib.testing():
        with case.device() as d:
            res = d.assignment_text_lz4(case.counts, thresh, case.names, prefix=prefix)
            plain = d.assignment_text(case.counts, thresh, case.names)
    assert plain.text.tobytes() == want.text.tobytes()
    f = check_result(res, want, prefix)
    assert res.raw_blocks == 0 and len(res.text) < res.content_bytes
    # The chunks follow from the line offsets: whole lines that fit the buffer, one line at the least; the first chunk
    # is the prefix, which leaves no room, and so one line.  Each chunk is cut into full blocks and a short last one.
    # (The short blocks may waste less than one block between them, so the block count alone shows nothing.)
    off = [int(o) for o in want.line_off]
    chunks, r0 = [], 0
    while r0 < len(off) - 1:
        r1 = max(int(np.searchsorted(want.line_off, off[r0] + (buf if chunks else 0), side="right")) - 1, r0 + 1)
        chunks.append((0 if chunks else len(prefix)) + off[r1] - off[r0])
        r0 = r1
    assert len(chunks) >= 5 and chunks[0] == len(prefix) + off[1] > buf
    lengths = [n for chunk in chunks for n in [BLOCK] * (chunk // BLOCK) + [chunk % BLOCK] if n]
    assert [b[2] for b in f.blocks] == lengths and sum(n < BLOCK for n in lengths) >= 5


def hand_built():
    rng = np.random.default_rng(5)
    n = 40
    sizes = [1 + i % 6 for i in range(n)]
    sizes[7] = 0
    row_ptr = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(sizes, out=row_ptr[1:])
    tid = np.concatenate([rng.choice(5000, size=k, replace=False) for k in sizes]).astype(np.uint32)
    as_prob = rng.uniform(0.1, 1.0, size=len(tid)).astype(np.float32)
    counts = rng.uniform(0.0, 30.0, size=5000)
    names = [f"r{i}".encode() * (1 + i % 3) for i in range(n)]
    return row_ptr, tid, as_prob, counts, names


@pytest.mark.parametrize("prefix_len", (0, 1, 65_535, 65_536, 65_537))
def test_prefix_lengths(prefix_len):
    row_ptr, tid, as_prob, counts, names = hand_built()
    rng = np.random.default_rng(prefix_len)
    prefix = b"".join(b"ENST%08d.%d\n" % (int(i), int(i) % 9) for i in rng.integers(0, 10 ** 8, size=prefix_len // 15 + 1))[:prefix_len]
    with DeviceStore(row_ptr, tid, as_prob, None, 5000) as d:
        want = d.assignment_text(counts, 1e-3, names)
        res = d.assignment_text_lz4(counts, 1e-3, names, prefix=prefix)
        bare = d.assignment_text_lz4(counts, 1e-3, None, prefix=prefix)
        bare_want = d.assignment_text(counts, 1e-3)
    f = check_result(res, want, prefix)
    assert len(want) == 40 and f.n_blocks == -(-(prefix_len + len(want.text)) // BLOCK)
    check_result(bare, bare_want, prefix)                      # names=None: every line starts with the tab


def test_store_without_reads():
    counts = np.array([1.0, 2.0, 4.0])
    with DeviceStore(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32), None, 3) as d:
        res = d.assignment_text_lz4(counts, 1e-3, [], prefix=b"3\t0\nA\nB\nC\n")
        f = lz.decode_everywhere(res.text.tobytes())
        assert f.content == b"3\t0\nA\nB\nC\n" and (res.content_bytes, res.n_blocks, res.raw_blocks) == (10, 1, 1)
        assert list(res.line_off) == [0] and len(res.kept) == 0
        res = d.assignment_text_lz4(counts, 1e-3, [])
        assert res.text.tobytes() == lz.frame_header(0) + bytes(4) and len(res.text) == 19
        assert lz.decode_everywhere(res.text.tobytes()).content == b""
        assert (res.content_bytes, res.n_blocks, res.raw_blocks) == (0, 0, 0)


def test_argument_errors_and_info():
    L = _lib.lib()
    rp = np.array([0, 2, 3], dtype=np.uint64)
    tid = np.array([0, 1, 2], np.uint32)
    counts = np.array([1.0, 2.0, 4.0])
    blob = np.frombuffer(b"abcd", dtype=np.uint8)
    off = np.array([0, 2, 4], dtype=np.uint64)
    pre = np.frombuffer(b"3\t2\n", dtype=np.uint8)

    def call(store, cnt, names, name_off, prefix, prefix_len, out):
        return L.oem_assignment_text_lz4(store, cnt, 1e-3, names, name_off, prefix, prefix_len, out)

    with DeviceStore(rp, tid, np.array([1.0, 0.5, 1.0], np.float32), None, 3) as d:
        cp = counts.ctypes.data
        for args, what in (((None, cp, None, None, None, 0), b"NULL argument"),
                           ((d.handle, None, None, None, None, 0), b"NULL argument"),
                           ((d.handle, cp, None, None, None, 4), b"prefix"),
                           ((d.handle, cp, blob.ctypes.data, None, None, 0), b"come together"),
                           ((d.handle, cp, None, off.ctypes.data, None, 0), b"come together")):
            h = C.c_void_p(1)
            assert call(*args, C.byref(h)) == _lib.OEM_ERR_ARG and h.value is None
            assert what in L.oem_last_error() and b"oem_assignment_text_lz4" in L.oem_last_error()
        assert call(d.handle, cp, None, None, None, 0, None) == _lib.OEM_ERR_ARG
        h = C.c_void_p()
        assert call(d.handle, cp, blob.ctypes.data, off.ctypes.data, pre.ctypes.data, 4, C.byref(h)) == _lib.OEM_OK and h.value
        p = C.c_void_p()
        assert L.oem_assignment_text(d.handle, cp, 1e-3, blob.ctypes.data, off.ctypes.data, C.byref(p)) == _lib.OEM_OK
    try:                                                       # the store is gone; the results are not
        v, nb = C.c_uint64(7), C.c_uint64(0)
        info = {}
        for r in (h, p):
            for key in (_lib.OEM_TEXT_INFO_CONTENT_BYTES, _lib.OEM_TEXT_INFO_BLOCKS, _lib.OEM_TEXT_INFO_RAW_BLOCKS):
                assert L.oem_text_result_info(r, key, C.byref(v)) == _lib.OEM_OK
                info[(r is h, key)] = v.value
        assert L.oem_text_result_dims(p, C.byref(nb), None, None) == _lib.OEM_OK and nb.value == 34
        assert [info[(False, k)] for k in (1, 2, 3)] == [34, 0, 0]
        assert [info[(True, k)] for k in (1, 2)] == [38, 1] and info[(True, 3)] in (0, 1)
        assert L.oem_text_result_info(h, 99, C.byref(v)) == _lib.OEM_ERR_ARG
        assert L.oem_text_result_info(None, 1, C.byref(v)) == _lib.OEM_ERR_ARG
        assert L.oem_text_result_info(h, 1, None) == _lib.OEM_ERR_ARG
        assert L.oem_text_result_dims(h, C.byref(nb), None, None) == _lib.OEM_OK
        frame = np.zeros(nb.value, dtype=np.uint8)
        assert L.oem_text_result_copy(h, frame.ctypes.data, None, None) == _lib.OEM_OK
        assert lz.decode_everywhere(frame.tobytes()).content == b"3\t2\nab\t2\t0\t1\t0.500\t0.500\ncd\t1\t2\t1.000\n"
    finally:
        L.oem_text_result_destroy(h)
        L.oem_text_result_destroy(p)


def test_writer_and_bulk_driver(tmp_path):
    """`<out>.prob.lz4` decodes to the bytes of the `<out>.prob` the same writer makes uncompressed, from the writer and
    through `BulkArgs.prob_on_device` + `prob_compressed` (compared on that run's own counts: two EM runs may differ in
    the last bits of a count)."""
    from oarfish_amd.bulk import BulkArgs, perform_inference_and_write_output
    st = synth.make_sirv_store("C", 20_000)
    names = [f"SIRV{i}" for i in range(st.n_txps)]
    lens = (500 + np.arange(st.n_txps) * 13 % 2500).tolist()
    rnames = [f"read/{i}" + ("\0" if i % 5 == 0 else "") for i in range(st.n_reads)]
    store = InMemoryAlignmentStore.from_arrays(st.row_ptr, st.tid, st.as_prob)
    out = str(tmp_path / "bulk" / "sample")
    args = BulkArgs(output=out, write_assignment_probs=True, display_thresh=1e-4, prob_on_device=True, prob_compressed=True)
    counts = perform_inference_and_write_output(store, names, lens, args, read_names=rnames)
    store.invalidate_device()
    with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, st.n_txps) as d:
        plain = open(writers.write_out_prob_device(str(tmp_path / "plain"), d, counts, rnames, names, 1e-4), "rb").read()
        path = writers.write_out_prob_device(str(tmp_path / "packed"), d, counts, rnames, names, 1e-4, compressed=True)
    assert path.endswith("packed.prob.lz4") and plain.count(b"\n") == st.n_txps + 1 + st.n_reads
    packed = open(path, "rb").read()
    assert lz.decode_everywhere(packed).content == plain and len(packed) < len(plain)
    assert open(out + ".prob.lz4", "rb").read() == packed
    # the host writer's compressed=True stays what it was: not this feature
    with pytest.raises(NotImplementedError):
        writers.write_out_prob(str(tmp_path / "host"), st.row_ptr, st.tid, np.zeros(len(st.tid)), rnames, names, 1e-4,
                               compressed=True)
