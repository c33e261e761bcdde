"""GPU tests of oem_count_matrix_text: the `.count.mtx` file formatted on the device.

The reference is existing code: every case compares the device bytes with the `.count.mtx` that
`writers.write_single_cell_output` writes for the same triplets (`writers.csr_triplets` of the CSR).  The cases with
knobs run in the test-only library, where OEM_MTX_BUF_BYTES cuts the entries into chunks and OEM_MTX_GRID_BLOCKS makes
a workgroup walk several tiles.

The value sets tests/test_shortest_f32.py holds the host build of oem_shortest_f32.h to (tests/shortest_f32_common.py)
run through the device build as well (test_host_value_sets_on_the_device): there each line's value field is also
compared with `writers.rust_display` computed in the test."""
import os

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth, writers
from oarfish_amd.em import count_matrix_text

from . import shortest_f32_common as sets
from .shortest_f32_common import as_f32, exponent_grid

pytestmark = pytest.mark.gpu

# a line of the greatest length: two u32 of 10 digits, two blanks, the longest f32 text (48, oem_shortest_f32.h), '\n'.
# A chunk is as many entries as the text buffer holds such lines; a workgroup's stage holds 256 of them.
MAX_LINE = 10 + 1 + 10 + 1 + 48 + 1
WIDE_T = 100_001


def reference(tmp_path, n_rows, n_txps, rows, cols, vals):
    """(header, body) of the file the existing writer makes of the triplets."""
    out = str(tmp_path / "ref")
    writers.write_single_cell_output(out, {}, [""] * n_txps, None, n_rows, rows, cols, vals)
    data = open(out + ".count.mtx", "rb").read()
    at = 0
    for _ in range(3):
        at = data.index(b"\n", at) + 1
    return data[:at], data[at:]


def check_against_writer(tmp_path, indptr, cols, vals, n_txps, row_base=0, **kw):
    indptr = np.asarray(indptr, dtype=np.uint64)
    rows, c, v = writers.csr_triplets(indptr, cols, vals)
    header, body = reference(tmp_path, row_base + len(indptr) - 1, n_txps, rows + np.uint32(row_base), c, v)
    res = count_matrix_text(indptr, cols, vals, n_txps, row_base=row_base, prefix=header, **kw)
    got = res.text.tobytes()
    if got != header + body:
        gl, wl = got.split(b"\n"), (header + body).split(b"\n")
        bad = next((i for i, (a, b) in enumerate(zip(gl, wl)) if a != b), min(len(gl), len(wl)))
        pytest.fail(f"line {bad}: device {gl[bad:bad + 1]!r}, writer {wl[bad:bad + 1]!r} ({len(got)} / {len(header + body)} bytes)")
    check_offsets(res, body)
    return res, body


def check_offsets(res, body):
    """line_off are the offsets of the newline-split body (after the prefix); kept is one per line."""
    lines = body.split(b"\n")[:-1]
    assert len(res.line_off) == len(lines) + 1 and res.line_off[0] == 0
    assert np.array_equal(res.line_off[1:].astype(np.int64), np.cumsum([len(l) + 1 for l in lines], dtype=np.int64))
    assert len(res.kept) == len(lines) and (res.kept == 1).all()
    assert res.content_bytes == len(res.text)


def hand_built():
    """5 cells, the first, the middle and the last empty; columns at both ends and across the digit counts."""
    vals = np.array([0.0, 1.0, 0.1, 0.5, 16777216.0, 1e-7, 0, 0, 0, 3e10], dtype=np.float32)
    vals.view(np.uint32)[6:9] = (0x00000001, 0x00800000, 0x7F7FFFFF)   # the least subnormal, FLT_MIN, FLT_MAX
    cols = np.array([0, 9, 99, 999, WIDE_T - 1, 0, 9998, 9999, 99_999, WIDE_T - 1], dtype=np.uint32)
    return np.array([0, 0, 5, 5, 10, 10], dtype=np.uint64), cols, vals


def test_hand_built_matrix(tmp_path):
    indptr, cols, vals = hand_built()
    _, body = check_against_writer(tmp_path, indptr, cols, vals, WIDE_T)
    assert body.split(b"\n")[:3] == [b"2 1 0", b"2 10 1", b"2 100 0.1"]
    assert body.split(b"\n")[6] == b"4 9999 0." + b"0" * 44 + b"1"
    assert body.split(b"\n")[9] == b"4 100001 30000000000"


def test_hand_built_matrix_with_a_row_base(tmp_path):
    """row_base 8 and 95 further single-entry cells: rows 9 .. 108, across 9 -> 10 and 99 -> 100."""
    indptr, cols, vals = hand_built()
    more = np.arange(1, 96, dtype=np.uint64) + indptr[-1]
    indptr = np.concatenate([indptr, more])
    cols = np.concatenate([cols, np.arange(95, dtype=np.uint32) * 1000])
    vals = np.concatenate([vals, (np.arange(95) / 7.0 + 0.25).astype(np.float32)])
    _, body = check_against_writer(tmp_path, indptr, cols, vals, WIDE_T, row_base=8)
    firsts = [int(l.split(b" ")[0]) for l in body.split(b"\n")[:-1]]
    assert firsts[0] == 10 and firsts[-1] == 108 and {99, 100} <= set(firsts)


def random_matrix(n, n_cells=7, n_txps=60_000, seed=0):
    rng = np.random.default_rng([n, seed])
    cuts = np.sort(rng.integers(0, n + 1, n_cells - 1))
    indptr = np.concatenate([[0], cuts, [n]]).astype(np.uint64)
    cols = rng.integers(0, n_txps, n).astype(np.uint32)
    vals = np.exp(rng.uniform(np.log(1e-6), np.log(5e4), n)).astype(np.float32)
    return indptr, cols, vals, n_txps


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513, 4097])
def test_workgroup_and_chunk_edges(n, tmp_path, monkeypatch):
    """The same bytes at the defaults (one chunk, one tile per workgroup) and, with two workgroups walking the tiles,
    with chunks of a sixth of the entries (six or seven chunks; fewer entries than six are one entry per chunk), with
    a text buffer of 100 greatest lines -- less than the 256 that one workgroup's stage holds -- and, up to 513
    entries, with the smallest buffer the code takes: anything below one greatest line counts as one line, one entry
    per chunk."""
    indptr, cols, vals, T = random_matrix(n)
    whole, body = check_against_writer(tmp_path, indptr, cols, vals, T)
    bufs = [MAX_LINE * max(n // 6, 1), MAX_LINE * 100] + ([1] if n <= 513 else [])
    monkeypatch.setenv("OEM_MTX_GRID_BLOCKS", "2")
    for buf in bufs:
        if n >= 6:
            assert -(-n // max(buf // MAX_LINE, 1)) >= 5 or buf == MAX_LINE * 100
        monkeypatch.setenv("OEM_MTX_BUF_BYTES", str(buf))
        with _lib.testing():
            parts = count_matrix_text(indptr, cols, vals, T, prefix=b"")
        assert parts.text.tobytes() == body, buf
        assert np.array_equal(parts.line_off, whole.line_off) and np.array_equal(parts.kept, whole.kept)


def test_host_text_grows_when_later_lines_are_longer(tmp_path, monkeypatch):
    """The host text is sized from the lines measured so far: short lines first, the longest last."""
    n = 600
    indptr = np.array([0, 100, 100, n], dtype=np.uint64)
    cols = np.concatenate([np.zeros(300), np.full(300, WIDE_T - 1)]).astype(np.uint32)
    vals = np.ones(n, dtype=np.float32)
    vals.view(np.uint32)[300:] = 0x80000001
    monkeypatch.setenv("OEM_MTX_BUF_BYTES", str(MAX_LINE * 50))
    with _lib.testing():
        check_against_writer(tmp_path, indptr, cols, vals, WIDE_T, row_base=4_000_000_000)


def test_emit_alignment(tmp_path):
    """The prefix never reaches the device (the host places it), so a prefix length moves no store; what moves a
    workgroup's range is the text before it.  The second workgroup's range starts at line_off[256]: the first
    entry's value is 1, 10, 0.5 or 0.25 (1, 2, 3, 4 bytes), which puts that start -- the text buffer itself is
    256-byte aligned -- at all four alignments modulo 4."""
    indptr, cols, vals, T = random_matrix(257)
    starts = set()
    for first in (1.0, 10.0, 0.5, 0.25):
        vals[0] = first
        res, body = check_against_writer(tmp_path, indptr, cols, vals, T)
        starts.add(int(res.line_off[256]) % 4)
        for plen in (0, 1, 2, 3, 5):
            pre = b"%" * plen
            r = count_matrix_text(indptr, cols, vals, T, prefix=pre)
            assert r.text.tobytes() == pre + body and np.array_equal(r.line_off, res.line_off)
    assert starts == {0, 1, 2, 3}


def test_every_exponent_on_the_device(tmp_path):
    """The device build of oem_shortest_f32.h against the writer, on the grid tests/test_shortest_f32.py holds the
    host build to; negatives too."""
    bits = exponent_grid()
    vals = as_f32(np.concatenate([bits, bits[::7] | np.uint32(0x80000000)]))
    cols = (np.arange(len(vals)) % 1000).astype(np.uint32)
    check_against_writer(tmp_path, [0, len(vals)], cols, vals, 1000)


# name -> (the set as tests/test_shortest_f32.py draws it, values there are rounded to f32; how many there must be)
HOST_SETS = {
    "random_bit_patterns": (sets.random_bit_patterns, 100_000),
    "em_counts": (lambda: sets.bits_of_f32(sets.em_counts()), 100_000),
    "integers": (lambda: sets.bits_of_f32(sets.integers()), 70_000),
    "eighths": (lambda: sets.bits_of_f32(sets.eighths()), 4096),
    "subnormal_ladder": (sets.subnormal_ladder, 1023),
    "powers_of_ten_neighbours": (sets.powers_of_ten_neighbours, 418),
    "specials_and_negatives": (sets.specials_and_negatives, 14),
}


@pytest.mark.parametrize("name", list(HOST_SETS))
def test_host_value_sets_on_the_device(name, tmp_path, monkeypatch):
    """A value set of the host build as a matrix of four cells (the second empty, the cuts off the workgroup tiles):
    the text is the writer's, and the value field of every line is `rust_display(x, f32=True)`, NaNs and infinities
    included as drawn.  The random patterns once more in the test-only library, in six or more chunks with two
    workgroups walking the tiles: the same bytes and line_off."""
    make, count = HOST_SETS[name]
    vals = as_f32(make())
    n = len(vals)
    assert n == count
    if name == "random_bit_patterns":
        assert np.isnan(vals).sum() > 100                     # (the infinities are in specials_and_negatives)
    n_txps = 60_000
    cols = (np.arange(n) * 7 % n_txps).astype(np.uint32)
    indptr = [0, n // 3 + 1, n // 3 + 1, n - n // 5, n]
    whole, body = check_against_writer(tmp_path, indptr, cols, vals, n_txps)
    fields = [l.split(b" ")[2] for l in body.split(b"\n")[:-1]]
    got = whole.text.tobytes().split(b"\n")[3:-1]
    assert len(got) == len(fields) == n
    for i, (x, line, f) in enumerate(zip(vals, got, fields)):
        want = writers.rust_display(x, f32=True).encode()
        assert line.split(b" ")[2] == want == f, (i, hex(int(vals.view(np.uint32)[i])), line)
    if name == "random_bit_patterns":
        buf = MAX_LINE * (n // 6)
        assert -(-n // (buf // MAX_LINE)) >= 6
        monkeypatch.setenv("OEM_MTX_BUF_BYTES", str(buf))
        monkeypatch.setenv("OEM_MTX_GRID_BLOCKS", "2")
        with _lib.testing():
            parts = count_matrix_text(indptr, cols, vals, n_txps, prefix=b"")
        assert parts.text.tobytes() == body
        assert np.array_equal(parts.line_off, whole.line_off) and np.array_equal(parts.kept, whole.kept)


def test_end_to_end_files(tmp_path):
    n_cells, T = 8, 200
    cell_off, row_ptr, tid, p = synth.make_cells(n_cells, 300, T, seed=77)
    indptr, cols, vals, _ = oarfish_amd.em_cells_sparse(cell_off, row_ptr, tid, p, None, T)
    assert len(vals) > n_cells
    info = {"quant": {"n_cells": n_cells}, "filter": "none"}
    features = [f"ENST{i:011d}.1" for i in range(T)]
    barcodes = [f"{'ACGT'[c % 4] * 16}-{c}" for c in range(n_cells)]
    a, b = str(tmp_path / "host" / "out"), str(tmp_path / "device" / "out")
    writers.write_single_cell_output(a, info, features, barcodes, n_cells, *writers.csr_triplets(indptr, cols, vals))
    writers.write_single_cell_output_device(b, info, features, barcodes, n_cells, indptr, cols, vals)
    assert sorted(os.listdir(tmp_path / "host")) == sorted(os.listdir(tmp_path / "device"))
    for ext in (".meta_info.json", ".count.mtx", ".features.txt", ".barcodes.txt"):
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext


def test_no_entries_at_all():
    pre = b"%%MatrixMarket matrix coordinate real general\n% written by sprs\n3 5 0\n"
    for indptr in ([0, 0, 0, 0], [0]):
        for prefix in (pre, b""):
            res = count_matrix_text(indptr, [], [], 5, prefix=prefix)
            assert res.text.tobytes() == prefix and list(res.line_off) == [0] and len(res.kept) == 0
