"""GPU tests of oem_assignment_text: the body of the `.prob` file formatted on the device.

The reference for the body is existing code: `writers.write_out_prob` on `DeviceStore.assignment_probs` (held to the
oracle by tests/test_gpu_parity.py::test_aux_counts_and_assignment_probs); the device text must equal the file it
writes, after its T + 1 header lines, byte for byte.  The one place the two differ by design -- 0/0, which the
reference prints as `NaN` -- has its expected bytes written out by hand (test_nan_literal).

That reference shares the device's own probabilities with the text, so a wrong kept set would cancel.  The edge cases
(tests/prob_edges_common.py: rounding ties at every decimal count, probabilities equal to the threshold, a kept -0.0,
the carry into the integer digit) take nothing from the device: their expected bytes are the oracle's probabilities
printed by Python (tests/test_prob_edges.py checks that side on the CPU)."""
import ctypes as C

import numpy as np
import pytest

from oarfish_amd import _lib, synth, writers
from oarfish_amd.types import DeviceStore, InMemoryAlignmentStore, pack_read_names
from oracle import c_oracle

from . import lz4_common
from . import prob_edges_common as pe

pytestmark = pytest.mark.gpu

THRESHOLDS = (1e-6, 1e-3, 0.2, 1e-12)
N_READS, N_TXPS = 70_000, 3_000


def python_body(tmp_path, st_row_ptr, st_tid, probs, names, n_txps, thresh) -> bytes:
    """What the existing writer puts after the header lines."""
    txp_names = [f"T{i}" for i in range(min(n_txps, 3))]      # (the header is not under test: keep it short)
    path = writers.write_out_prob(str(tmp_path / "ref"), st_row_ptr, st_tid, probs, names, txp_names, thresh)
    data = open(path, "rb").read()
    at = 0
    for _ in range(len(txp_names) + 1):
        at = data.index(b"\n", at) + 1
    return data[at:]


def check_offsets(res, n_reads):
    """line_off and kept describe the text: every line ends at the next one's offset with a newline and has
    name, k, k ids and k probabilities."""
    text = res.text.tobytes()
    assert len(res.line_off) == n_reads + 1 and len(res.kept) == n_reads
    assert res.line_off[0] == 0 and res.line_off[-1] == len(text)
    lines = text.split(b"\n")
    assert lines[-1] == b"" and len(lines) == n_reads + 1
    assert np.array_equal(np.cumsum([len(l) + 1 for l in lines[:-1]]), res.line_off[1:].astype(np.int64))
    for r, line in enumerate(lines[:-1]):
        f = line.split(b"\t")
        k = int(f[1])
        assert k == res.kept[r]
        assert len(f) == (2 + 2 * k if k else 4), (r, line)


class Case:
    def __init__(self, coverage):
        self.st = synth.make_store(N_READS, N_TXPS, 4.0, seed=411 + coverage, coverage=bool(coverage))
        self.names = [f"read/{i:x}" + ("#" * (i % 7)) for i in range(N_READS)]
        with self.device() as d:
            self.counts, _ = d.em_run(None, 120, 1e-3, 50)
        assert (self.counts == 0.0).sum() > 0        # zeroed transcripts: their alignments drop out

    def device(self):
        st = self.st
        return DeviceStore(st.row_ptr, st.tid, st.as_prob, st.cov_prob, st.n_txps)


_cases = {}


@pytest.fixture(scope="module", params=[0, 1], ids=["plain", "coverage"])
def case(request):
    if request.param not in _cases:
        _cases[request.param] = Case(request.param)
    return _cases[request.param]


@pytest.mark.parametrize("thresh", THRESHOLDS)
def test_text_equals_the_python_writer_byte_for_byte(case, thresh, tmp_path):
    st = case.st
    with case.device() as d:
        probs = d.assignment_probs(case.counts, thresh)
        res = d.assignment_text(case.counts, thresh, case.names)
    want = python_body(tmp_path, st.row_ptr, st.tid, probs, case.names, st.n_txps, thresh)
    got = res.text.tobytes()
    if got != want:
        gl, wl = got.split(b"\n"), want.split(b"\n")
        bad = next(i for i, (a, b) in enumerate(zip(gl, wl)) if a != b)
        pytest.fail(f"line {bad}: device {gl[bad]!r} != python {wl[bad]!r}")
    lo = st.row_ptr[:-1].astype(np.int64)
    assert np.array_equal(res.kept, np.add.reduceat((probs >= 0).astype(np.int64), lo))
    assert int(res.line_off[-1]) == len(want)
    if thresh == 0.2:
        check_offsets(res, st.n_reads)
        assert res.kept.max() > 1


IDS = (0, 9, 10, 99_999, 100_000, 1_234_567)
WIDE_T = 1_234_568


def hand_built():
    rng = np.random.default_rng(5)
    rows, names = [], []
    zero = (5, 6, 7)

    def add(ids, name):
        rows.append(np.asarray(ids, dtype=np.uint32))
        names.append(name)

    for n in (1, 9, 10, 99, 100):                             # k with one to three digits
        ids = rng.choice(np.arange(1000, WIDE_T), size=n, replace=False)
        add(ids, f"k{n}".encode())
    add([], b"empty-row")
    add(IDS, b"")                                             # id lengths 1 .. 7, a name of length 0
    add([3, 4], b"x")
    add([11, 12, 13], b"trailing\0\0\0")
    add([100, 200], bytes(33 + (i % 90) for i in range(300)))  # longer than a staging slot
    add(zero, b"no-mass")                                     # denom = 0: NaN nprob, nothing kept
    add([5, 42], b"half-mass")
    add([], b"")
    for i in range(30):                                       # filler around them, 1 .. 6 alignments
        add(rng.choice(np.arange(8, 5000), size=1 + i % 6, replace=False), f"r{i}".encode() * (1 + i % 3))
    row_ptr = np.zeros(len(rows) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in rows], out=row_ptr[1:])
    tid = np.concatenate(rows).astype(np.uint32)
    as_prob = rng.uniform(0.1, 1.0, size=len(tid)).astype(np.float32)
    counts = np.ones(WIDE_T)
    counts[list(zero)] = 0.0
    counts[rng.integers(300, 5000, size=400)] = rng.uniform(0.0, 30.0, size=400)
    return row_ptr, tid, as_prob, counts, names


def test_hand_built_store(tmp_path):
    row_ptr, tid, as_prob, counts, names = hand_built()
    n = len(names)
    str_names = [b.decode("latin-1") for b in names]
    with DeviceStore(row_ptr, tid, as_prob, None, WIDE_T) as d:
        for thresh in (1e-6, 1e-3, 0.2):
            probs = d.assignment_probs(counts, thresh)
            res = d.assignment_text(counts, thresh, names)
            want = python_body(tmp_path, row_ptr, tid, probs, str_names, WIDE_T, thresh)
            # (the writer encodes its str names as UTF-8; the names here are ASCII, so latin-1 round-trips them)
            assert res.text.tobytes() == want, thresh
            check_offsets(res, n)
        res = d.assignment_text(counts, 1e-6, names)
        lines = res.text.tobytes().split(b"\n")
        assert [int(res.kept[i]) for i in range(5)] == [1, 9, 10, 99, 100]
        assert lines[5] == b"empty-row\t0\t\t" and lines[12] == b"\t0\t\t" and lines[10] == b"no-mass\t0\t\t"
        assert lines[6].split(b"\t")[:8] == [b"", b"6"] + [str(i).encode() for i in IDS]
        assert lines[8].startswith(b"trailing\t3\t11\t12\t13\t") and lines[9].startswith(names[9] + b"\t2\t100\t200\t")
        assert lines[11].startswith(b"half-mass\t1\t42\t1.000000")
        # no names at all: every line starts with the tab; and the (blob, offsets) form of the names
        bare = d.assignment_text(counts, 1e-6)
        assert bare.text.tobytes().split(b"\n")[:-1] == [l[l.index(b"\t"):] for l in lines[:-1]]
        pair = d.assignment_text(counts, 1e-6, pack_read_names(names, n))
        assert pair.text.tobytes() == res.text.tobytes()


@pytest.mark.parametrize("thresh,decimals", [(1e-4, 4), (1e-5, 5), (1e-7, 7), (1e-8, 8)])
def test_hand_built_store_at_the_other_decimal_counts(thresh, decimals, tmp_path):
    """test_hand_built_store prints with 6, 3 and 3 decimals; these are the counts in between."""
    row_ptr, tid, as_prob, counts, names = hand_built()
    str_names = [b.decode("latin-1") for b in names]
    assert writers.prob_display_decimals(thresh) == decimals
    with DeviceStore(row_ptr, tid, as_prob, None, WIDE_T) as d:
        probs = d.assignment_probs(counts, thresh)
        res = d.assignment_text(counts, thresh, names)
    assert res.text.tobytes() == python_body(tmp_path, row_ptr, tid, probs, str_names, WIDE_T, thresh)
    check_offsets(res, len(names))
    assert res.line(11) == b"half-mass\t1\t42\t1." + b"0" * decimals + b"\n"


_edges = {}


def edge_case():
    """The edge store and, once for the module, the oracle's probabilities and the expected text at every threshold."""
    if not _edges:
        st = pe.EdgeStore()
        pe.assert_exact(st)
        o = c_oracle.Store(st.row_ptr, st.tid, st.as_prob, None, st.n_txps)
        want = {}
        for thresh in pe.THRESHOLDS:
            probs = c_oracle.assignment_probs(o, st.counts, thresh)
            want[thresh] = (probs,) + pe.expected_text(st, probs, thresh, st.names)
        _edges.update(st=st, want=want)
    return _edges["st"], _edges["want"]


def assert_same_text(res, body, line_off, kept, what):
    got = res.text.tobytes()
    if got != body:
        gl, wl = got.split(b"\n"), body.split(b"\n")
        bad = next((i for i, (a, b) in enumerate(zip(gl, wl)) if a != b), min(len(gl), len(wl)))
        pytest.fail(f"{what}: line {bad}: device {gl[bad:bad + 1]!r}, expected {wl[bad:bad + 1]!r}")
    assert np.array_equal(res.line_off, line_off) and np.array_equal(res.kept, kept), what


@pytest.mark.parametrize("thresh", pe.THRESHOLDS, ids=repr)
def test_edge_store_equals_the_oracle_printed_by_python(thresh):
    """Ties (d = 3 .. 9), threshold equality and its two neighbours (0.2, 0.25, 0.5), -0.0 and the carry (0): the
    device's probabilities are the oracle's bit for bit, -1 markers included, and text, line_off and kept are what
    Python's formatting makes of the oracle's probabilities."""
    st, want = edge_case()
    probs, body, line_off, kept = want[thresh]
    with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, st.n_txps) as d:
        got_probs = d.assignment_probs(st.counts, thresh)
        res = d.assignment_text(st.counts, thresh, st.names)
    assert np.array_equal(got_probs, probs) and np.array_equal(np.signbit(got_probs), np.signbit(probs))
    assert_same_text(res, body, line_off, kept, thresh)
    pe.check_edge_lines(st, thresh, res.text.tobytes(), res.line_off, res.kept)
    check_offsets(res, st.n_reads)


@pytest.mark.parametrize("thresh", [0.0, 1e-3, pe.around(0.2)[2]], ids=repr)
def test_edge_store_in_chunks_and_compressed(thresh, monkeypatch):
    """The same expected bytes from the chunked call (four or more chunks, two workgroups striding over each) and,
    decoded, from the compressed call; 0 has the signs and the carry, 1e-3 the d = 3 ties, the neighbour above 0.2
    the lines that keep nothing."""
    st, want = edge_case()
    _, body, line_off, kept = want[thresh]
    buf = len(body) // 4 - 50
    assert len(body) > 4 * buf and buf > 200
    prefix = b"%d\t%d\n" % (st.n_txps, st.n_reads)
    with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, st.n_txps) as d:
        frame = d.assignment_text_lz4(st.counts, thresh, st.names, prefix=prefix)
    assert lz4_common.decode_everywhere(frame.text.tobytes()).content == prefix + body
    assert np.array_equal(frame.line_off, line_off) and np.array_equal(frame.kept, kept)
    monkeypatch.setenv("OEM_TEXT_BUF_BYTES", str(buf))
    monkeypatch.setenv("OEM_TEXT_GRID_BLOCKS", "2")
    with _lib.testing():
        with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, st.n_txps) as d:
            parts = d.assignment_text(st.counts, thresh, st.names)
            bare = d.assignment_text(st.counts, thresh)
    assert_same_text(parts, body, line_off, kept, "chunks")
    assert bare.text.tobytes().split(b"\n") == [l[l.index(b"\t"):] if l else l for l in body.split(b"\n")]


def test_nan_literal():
    """write_function.rs:307-318 with display_thresh = 0: a read whose denom is +inf (two alignments of 1e308 each)
    has every nprob = x / inf = 0, all kept (0 >= 0), denom2 = 0, so every printed value is 0 / 0.  Rust's `{:.9}`
    prints `NaN`.  (A read that merely has count 0 on all its transcripts has denom = 0, NaN nprob, and keeps
    nothing; and a read with one positive finite term keeps it at 1.)  The expected bytes are written out here: the
    Python path cannot serve as the reference for this line -- `assignment_probs` hands it NaN where the -1 marker
    would be, and its `probs >= 0` mask then drops the three alignments."""
    row_ptr = np.array([0, 3, 5, 7], dtype=np.uint64)
    tid = np.array([0, 1, 2, 3, 4, 3, 2], dtype=np.uint32)
    as_prob = np.array([1.0, 1.0, 0.5, 1.0, 0.5, 0.25, 1.0], dtype=np.float32)
    counts = np.array([1e308, 1e308, 7.0, 0.0, 0.0])
    with DeviceStore(row_ptr, tid, as_prob, None, 5) as d:
        res = d.assignment_text(counts, 0.0, ["inf", "zero", "one"])
        probs = d.assignment_probs(counts, 0.0)
    assert float(counts[0]) + float(counts[1]) == float("inf") and np.all(np.isnan(probs[:3]))
    lines = res.text.tobytes().split(b"\n")
    assert lines[0] == b"inf\t3\t0\t1\t2\tNaN\tNaN\tNaN"
    assert lines[1] == b"zero\t0\t\t"
    assert lines[2] == b"one\t2\t3\t2\t0.000000000\t1.000000000"
    assert list(res.kept) == [3, 0, 2] and lines[3] == b"" and len(lines) == 4
    # what Python's own float formatting makes of the same values, lower-cased as its `nan` is
    assert lines[0].lower().split(b"\t")[5:] == [f"{x:.9f}".encode() for x in probs[:3]]


def test_chunks_give_the_same_text(case, monkeypatch):
    thresh = 1e-3
    with case.device() as d:
        whole = d.assignment_text(case.counts, thresh, case.names)
    n_bytes = len(whole.text)
    buf = 1 << 18
    assert n_bytes > 4 * buf                                  # four or more chunks
    monkeypatch.setenv("OEM_TEXT_BUF_BYTES", str(buf))
    monkeypatch.setenv("OEM_TEXT_GRID_BLOCKS", "16")          # 4096 lanes: several grid strides per chunk
    with _lib.testing():
        with case.device() as d:
            parts = d.assignment_text(case.counts, thresh, case.names)
    assert parts.text.tobytes() == whole.text.tobytes()
    assert np.array_equal(parts.line_off, whole.line_off) and np.array_equal(parts.kept, whole.kept)
    # a buffer smaller than one line: the 300-byte name's read still comes out right
    row_ptr, tid, as_prob, counts, names = hand_built()
    with DeviceStore(row_ptr, tid, as_prob, None, WIDE_T) as d:
        want = d.assignment_text(counts, 1e-6, names)
    monkeypatch.setenv("OEM_TEXT_BUF_BYTES", "128")
    monkeypatch.delenv("OEM_TEXT_GRID_BLOCKS")
    with _lib.testing():
        with DeviceStore(row_ptr, tid, as_prob, None, WIDE_T) as d:
            got = d.assignment_text(counts, 1e-6, names)
    assert got.text.tobytes() == want.text.tobytes() and len(want.line(9)) > 300


@pytest.mark.parametrize("kind", ["f32_stream", "coverage_f32", "with_coverage"])
def test_kinds_of_store(kind, tmp_path):
    """weight_coding 1, a weight_coding 2 coverage store (f32 products) and a store whose coverage column was computed on
    the device: each store's text equals its own assignment_probs through the Python writer."""
    n_reads, n_txps = 20_000, 2_000
    st = synth.make_store(n_reads, n_txps, 4.0, seed=97, coverage=(kind == "coverage_f32"))
    if kind == "f32_stream":
        d = DeviceStore(st.row_ptr, st.tid, st.as_prob, None, n_txps, weight_coding=1)
    elif kind == "coverage_f32":
        d = DeviceStore(st.row_ptr, st.tid, st.as_prob, st.cov_prob, n_txps, weight_coding=2)
    else:
        txp_len, a0, a1 = synth.make_coordinates(st.tid, n_txps)
        d = DeviceStore.with_coverage(st.row_ptr, st.tid, st.as_prob, a0, a1, txp_len)
    names = [f"m{i}" for i in range(n_reads)]
    with d:
        counts, _ = d.em_run(None, 60, 1e-3, 50)
        for thresh in (1e-6, 0.2):
            probs = d.assignment_probs(counts, thresh)
            res = d.assignment_text(counts, thresh, names)
            assert res.text.tobytes() == python_body(tmp_path, st.row_ptr, st.tid, probs, names, n_txps, thresh), thresh


def test_argument_errors_and_lifetime():
    L = _lib.lib()
    rp = np.array([0, 2, 3], dtype=np.uint64)
    tid = np.array([0, 1, 2], np.uint32)
    counts = np.array([1.0, 2.0, 4.0])
    blob = np.frombuffer(b"abcd", dtype=np.uint8)
    off = np.array([0, 2, 4], dtype=np.uint64)

    def call(store, cnt, names, name_off, out):
        return L.oem_assignment_text(store, cnt, 1e-3, names, name_off, out)

    with DeviceStore(rp, tid, np.array([1.0, 0.5, 1.0], np.float32), None, 3) as d:
        h = C.c_void_p(1)
        assert call(None, counts.ctypes.data, None, None, C.byref(h)) == _lib.OEM_ERR_ARG and h.value is None
        h = C.c_void_p(1)
        assert call(d.handle, None, None, None, C.byref(h)) == _lib.OEM_ERR_ARG and h.value is None
        assert call(d.handle, counts.ctypes.data, None, None, None) == _lib.OEM_ERR_ARG
        off_from_1, off_decreasing = np.array([1, 2, 4], np.uint64), np.array([0, 3, 2], np.uint64)   # (alive during the calls)
        for names, name_off, what in ((blob.ctypes.data, None, b"come together"), (None, off.ctypes.data, b"come together"),
                                      (blob.ctypes.data, off_from_1.ctypes.data, b"name_off[0]"),
                                      (blob.ctypes.data, off_decreasing.ctypes.data, b"non-decreasing")):
            h = C.c_void_p(1)
            assert call(d.handle, counts.ctypes.data, names, name_off, C.byref(h)) == _lib.OEM_ERR_ARG
            assert h.value is None and what in L.oem_last_error()
        L.oem_text_result_destroy(None)                        # a no-op
        assert L.oem_text_result_dims(None, None, None, None) == _lib.OEM_ERR_ARG
        assert L.oem_text_result_copy(None, None, None, None) == _lib.OEM_ERR_ARG
        h = C.c_void_p()
        assert call(d.handle, counts.ctypes.data, blob.ctypes.data, off.ctypes.data, C.byref(h)) == _lib.OEM_OK and h.value
    # the store is gone; the result is not
    try:
        nb, nl, nk = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        assert L.oem_text_result_dims(h, C.byref(nb), C.byref(nl), C.byref(nk)) == _lib.OEM_OK
        assert (nl.value, nk.value) == (2, 3)
        text = np.zeros(nb.value, dtype=np.uint8)
        lo = np.zeros(3, dtype=np.uint64)
        kept = np.zeros(2, dtype=np.uint32)
        assert L.oem_text_result_copy(h, text.ctypes.data, lo.ctypes.data, kept.ctypes.data) == _lib.OEM_OK
        assert text.tobytes() == b"ab\t2\t0\t1\t0.500\t0.500\ncd\t1\t2\t1.000\n"
        assert list(lo) == [0, 21, 34] and list(kept) == [2, 1]
        assert L.oem_text_result_copy(h, text.ctypes.data, None, None) == _lib.OEM_OK
    finally:
        L.oem_text_result_destroy(h)
    # an empty store: no lines, one offset
    with DeviceStore(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32), None, 3) as d:
        res = d.assignment_text(counts, 1e-3, [])
        assert len(res.text) == 0 and list(res.line_off) == [0] and len(res.kept) == 0


def test_bulk_driver_writes_the_same_prob_file(tmp_path):
    """bulk.rs:196-207 through `BulkArgs.prob_on_device`: the file is the default path's.  The default path is
    `assignment_probs` + `write_out_prob` on the run's counts; two EM runs may differ in the last bits of a count (the
    order of the device's atomic sums), so the device file is compared with those two calls on ITS run's counts, and
    with the default run's file whenever the two runs' counts are bitwise equal."""
    from oarfish_amd.bulk import BulkArgs, perform_inference_and_write_output
    st = synth.make_sirv_store("C", 20_000)
    names = [f"SIRV{i}" for i in range(st.n_txps)]
    lens = (500 + np.arange(st.n_txps) * 13 % 2500).tolist()
    rnames = [f"read/{i}" + ("\0" if i % 5 == 0 else "") for i in range(st.n_reads)]
    files, counts = [], []
    for on_device in (False, True):
        store = InMemoryAlignmentStore.from_arrays(st.row_ptr, st.tid, st.as_prob)
        out = str(tmp_path / ("dev" if on_device else "host") / "sample")
        args = BulkArgs(output=out, write_assignment_probs=True, display_thresh=1e-4, prob_on_device=on_device)
        counts.append(perform_inference_and_write_output(store, names, lens, args, read_names=rnames))
        files.append(open(out + ".prob", "rb").read())
        store.invalidate_device()
    with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, st.n_txps) as d:
        probs = d.assignment_probs(counts[1], 1e-4)
    want = open(writers.write_out_prob(str(tmp_path / "want"), st.row_ptr, st.tid, probs, rnames, names, 1e-4), "rb").read()
    assert files[1] == want and files[1].count(b"\n") == st.n_txps + 1 + st.n_reads
    assert files[0].split(b"\n")[:st.n_txps + 1] == files[1].split(b"\n")[:st.n_txps + 1]
    if np.array_equal(counts[0], counts[1]):
        assert files[0] == files[1]
