"""The any-order barcoded cells session, without a device: the streamed rule of oem_collate.h (ParseCellsAnyOrderStream,
with the host form of the barcode table of oem_barcode_table.h) against the barcode rule's host walk on every cutting of
a small input and on seeded random inputs, under the sanitizers; the cutter; the ABI's shape; the calls' argument and
state errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth
from oarfish_amd import build as _b
from oarfish_amd.builder import ALN_RECORD, REC_UNMAPPED
from oarfish_amd.em import CellsStream
from oarfish_amd.types import pack_read_names

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "parse_cells_any_order_main.cpp")
EXE = os.path.join(HERE, "native", "parse_cells_any_order_main")
HDRS = [os.path.join(ROOT, "oarfish_amd", "csrc", h) for h in ("oem_collate.h", "oem_barcode_table.h")]
NAME = "oem_cells_stream_set_barcodes_any_order"
FILTERS = dict(five_prime_clip=2 ** 32 - 1, three_prime_clip=2 ** 62, score_threshold=0.95, min_aligned_fraction=0.5,
               min_aligned_len=50, which_strand=0, score_prob_denom=5.0)
T = 8
U = REC_UNMAPPED
P9, Q9 = b"AAAAAAAAC", b"AAAAAAAAG"   # they first differ in byte 9: in the second 8-byte word of the comparison
C8 = b"CCCCCCCC"
GARBAGE = b"\x00\xff"
# 12 records, 6 barcodes, first seen in the REVERSE of their byte order.  T (1 byte) recurs after four other cells, C8
# (8 bytes) and ACGT-1 come back too; ACGT sits beside ACGT-1; one unmapped record leads the stream, one sits inside.
INPUT12 = [(U, GARBAGE), (0, b"T"), (0, C8), (0, b"ACGT-1"), (0, b"ACGT"), (0, b"T"), (0, Q9), (U, GARBAGE), (0, P9),
           (0, b"ACGT-1"), (0, Q9), (0, C8)]
SURVIVORS12 = [1, 2, 3, 4, 5, 6, 8, 9, 10, 11]
LABELS12 = [b"T", C8, b"ACGT-1", b"ACGT", Q9, P9]
ORDER12 = [0, 4, 1, 9, 2, 7, 3, 5, 8, 6]          # positions among the survivors, cell-major
CELLS12 = [0, 2, 4, 6, 7, 9, 10]


def test_the_input_is_what_the_issue_asks_for():
    assert len(INPUT12) == 12 and [f for f, _ in INPUT12].count(U) == 2 and INPUT12[0] == (U, GARBAGE) and INPUT12[7] == (U, GARBAGE)
    surv = [bc for f, bc in INPUT12 if not f]
    first_seen = list(dict.fromkeys(surv))
    assert first_seen == LABELS12 == sorted(LABELS12, reverse=True)            # byte order reversed
    assert surv.index(b"T") == 0 and surv[4] == b"T" and surv[1:4] != [b"T"] * 3  # recurs after other cells
    assert b"ACGT" in LABELS12 and b"ACGT-1" in LABELS12
    assert P9[:8] == Q9[:8] and len(P9) == len(Q9) == 9 and P9 != Q9
    assert {1, 8} <= {len(b) for b in LABELS12}
    assert [SURVIVORS12[k] for k in ORDER12] == [i for lab in LABELS12 for i in SURVIVORS12 if INPUT12[i][1] == lab]
    assert len(LABELS12) >= 5      # a first capacity of 2 doubles three times: 2 -> 4 -> 8 -> 16


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-o", EXE, SRC])
    return EXE


def test_interned_cells_equal_the_barcode_walk_for_every_cutting_and_table_under_sanitizers(exe):
    text = f"{len(INPUT12)}\n" + "".join(f"{f} {bc.hex() or '-'}\n" for f, bc in INPUT12)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    head, rebuilds = r.stdout.strip().rsplit(" | ", 1)
    want = ("ok 2048 6 2 | " + " ".join(map(str, CELLS12)) + " | " + " ".join(b.hex() for b in LABELS12) + " | "
            + " ".join(map(str, ORDER12)) + " | " + " ".join(map(str, SURVIVORS12)))
    assert head == want
    # one record per batch: the default table never grows, a first capacity of 2 doubles at the 2nd, 3rd and 5th label
    assert rebuilds.split() == ["0", "3", "3", "3"]


def test_seeded_random_inputs_under_random_cuttings(exe):
    for seed in (1, 2, 3):
        r = subprocess.run([exe, "random", str(seed), "400"], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("ok 400 "), (r.stdout, r.stderr[-2000:])


def test_declared_exported_by_both_libraries_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "oarfish_em.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, src)
    assert m, "include/oarfish_em.h does not declare " + NAME
    assert len(m.group(1).split(",")) == 2
    assert NAME in _lib.ABI_SYMBOLS and len(getattr(_lib.lib(), NAME).argtypes) == 2
    for path in (_b.LIB_PATH, _b.TESTING_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert NAME in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, path
    assert "oem_debug_barcode_table_last" in _b.TESTING_HOOKS
    assert "#define OEM_ABI_VERSION 2" in src and C.sizeof(_lib.CellsStreamOptsC) == 88   # the options are not touched
    full = open(os.path.join(ROOT, "include", "oarfish_em.h")).read()
    for key, v in (("ARENA_BYTES", 7), ("BARCODE_MISSES", 8), ("BARCODE_TABLE_SLOTS", 9)):
        assert f"OEM_CELLS_STREAM_INFO_{key} {v}u" in full and getattr(_lib, "OEM_CELLS_STREAM_INFO_" + key) == v
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read(), "INTEGRATION.md does not name " + NAME
    rule = open(HDRS[0]).read()
    assert "Cells from a stream in any order" in rule and "struct ParseCellsAnyOrderStream" in rule
    assert "oem_cells_barcodes_sort_stream.hip" in _b.SOURCES and "oem_barcode_table.h" in _b.HEADERS


def test_null_sessions_and_sessions_without_a_device():
    L = _lib.lib()
    assert L.oem_cells_stream_set_barcodes_any_order(None, 0) == _lib.OEM_ERR_ARG and b"NULL session" in L.oem_last_error()
    assert L.oem_cells_stream_set_barcodes_any_order(None, 7) == _lib.OEM_ERR_ARG
    v = C.c_uint64(5)
    assert L.oem_cells_stream_info(None, _lib.OEM_CELLS_STREAM_INFO_BARCODE_MISSES, C.byref(v)) == _lib.OEM_ERR_ARG and v.value == 5
    if _lib.device_count() > 0:
        return
    with pytest.raises(_lib.OemError) as ei:
        CellsStream(T, filters=FILTERS, txp_len=np.full(T, 2000, dtype=np.uint64), barcodes=True, collated=False)
    assert ei.value.code == _lib.OEM_ERR_NO_DEVICE


def test_the_wrapper_checks_its_own_arguments():
    with pytest.raises(ValueError, match="collated"):
        CellsStream(T, collated=False)
    with pytest.raises(ValueError, match="collated"):
        CellsStream(T, filters=FILTERS, txp_len=np.full(T, 2000, dtype=np.uint64), collated=False)
    with pytest.raises(ValueError, match="filters"):
        CellsStream(T, barcodes=True, collated=False)
    with pytest.raises(ValueError, match="mode"):
        CellsStream(T, filters=FILTERS, txp_len=np.full(T, 2000, dtype=np.uint64), barcodes=True, collated=False, mode="sorted")
    from oarfish_amd.single_cell import SingleCellArgs
    assert SingleCellArgs(output="x").collated is True and SingleCellArgs(output="x", collated=False).collated is False


def _join(batches):
    rec = np.concatenate([b[0] for b in batches])
    out = [rec]
    for k in (1, 2):
        blob = np.concatenate([b[k][0] for b in batches])
        lens = np.concatenate([np.diff(b[k][1].astype(np.int64)) for b in batches])
        out.append([blob.tobytes()[a:a + l] for a, l in zip(np.cumsum(lens) - lens, lens)])
    out.append(np.concatenate([b[3] for b in batches]))
    return out


def _unpack(pair):
    raw, off = np.asarray(pair[0], dtype=np.uint8).tobytes(), np.asarray(pair[1], dtype=np.int64)
    return [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]


@pytest.mark.parametrize("how", ["uniform", "blocks"])
def test_cut_interleaved_records_round_trips(how):
    n_cells, per_cell = 4, 5
    n = n_cells * per_cell
    rec = np.zeros(n, dtype=ALN_RECORD)
    rec["ref_id"] = np.arange(n) % T
    rec["aln_start"] = np.arange(n)
    names = pack_read_names([b"r%d" % (i // 2) for i in range(n)], n)
    sec = (np.arange(n) % 2).astype(np.uint8)
    cro = np.arange(n_cells + 1, dtype=np.uint64) * per_cell
    bcs = synth.make_barcodes(n_cells)
    irec, inames, isec, ibc, perm = synth.interleave_cells(rec, names, sec, cro, bcs, seed=3, how=how)
    want_names, want_bc = _unpack(inames), _unpack(ibc)
    assert want_bc == [bcs[int(p) // per_cell].encode() if isinstance(bcs[0], str) else bcs[int(p) // per_cell] for p in perm]
    for cuts in [(), (0,), (n,), (5,), (7, 7), (13, 2), (0, 0, n, n), tuple(range(1, n))]:
        batches = synth.cut_interleaved_records(irec, inames, isec, ibc, cuts)
        assert len(batches) == len(cuts) + 1
        assert [len(b[0]) for b in batches] == list(np.diff([0] + sorted(cuts) + [n]))
        for b in batches:
            assert b[1][1][0] == 0 and b[2][1][0] == 0 and len(b[1][1]) == len(b[0]) + 1 == len(b[2][1]) and len(b[3]) == len(b[0])
            assert b[1][1].dtype == np.uint64 and b[2][1].dtype == np.uint64
        r, bc, nm, s = _join(batches)
        assert r.tobytes() == irec.tobytes() and bc == want_bc and nm == want_names and np.array_equal(s, isec)
    batches = synth.cut_interleaved_records(irec, inames, isec, ibc, (1, 9, 9, 20), unmapped_every=3)
    r, bc, nm, s = _join(batches)
    un = (r["flags"] & U) != 0
    assert len(r) == n + (n + 2) // 3 and un.sum() == (n + 2) // 3 and un[0] and [len(b[0]) for b in batches] == [1, 8, 0, 11, len(r) - 20]
    assert all(not bc[i] and not nm[i] for i in np.flatnonzero(un))
    keep = np.flatnonzero(~un)
    assert r[keep].tobytes() == irec.tobytes() and [bc[i] for i in keep] == want_bc and [nm[i] for i in keep] == want_names
    assert np.array_equal(s[keep], isec)
    with pytest.raises(ValueError):
        synth.cut_interleaved_records(irec, inames, isec, ibc, (n + 1,))
    with pytest.raises(ValueError):
        synth.cut_interleaved_records(irec, inames, isec, (ibc[0], ibc[1][:-1]), ())
    assert "cut_interleaved_records" in oarfish_amd.__all__
