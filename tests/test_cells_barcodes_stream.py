"""The barcoded cells session, without a device: the streamed cell rule of oem_collate.h (ParseCellsStream) on every
cutting of a small input, under the sanitizers; the cutter; the ABI's shape; the calls' argument and state errors."""
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

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "parse_cells_stream_main.cpp")
EXE = os.path.join(HERE, "native", "parse_cells_stream_main")
HDR = os.path.join(ROOT, "oarfish_amd", "csrc", "oem_collate.h")
NEW = ["oem_cells_stream_set_barcodes", "oem_cells_stream_push_barcodes", "oem_cells_stream_barcodes_dims",
       "oem_cells_stream_barcodes_copy"]
FILTERS = dict(five_prime_clip=2 ** 32 - 1, three_prime_clip=2 ** 62, score_threshold=0.95, min_aligned_fraction=0.5,
               min_aligned_len=50, which_strand=0, score_prob_denom=5.0)
T = 8
U = REC_UNMAPPED
P9, Q9 = b"AAAAAAAAC", b"AAAAAAAAG"   # they first differ in byte 9: in the second 8-byte word of the comparison
# 12 records, 4 barcodes.  ACGT recurs after ACGT-1, so the runs are five cells; ACGT-1 is a cell of one record; one
# unmapped record sits inside a cell, the other on a cell boundary with bytes no survivor may carry.
INPUT12 = [(0, b"ACGT"), (0, b"ACGT"), (U, b""), (0, b"ACGT"), (0, b"ACGT-1"), (0, b"ACGT"), (0, b"ACGT"),
           (U, b"\x00\xff"), (0, P9), (0, P9), (0, Q9), (0, Q9)]
CELLS12 = [0, 3, 4, 6, 8, 10]
LABELS12 = [b"ACGT", b"ACGT-1", b"ACGT", P9, Q9]
SURVIVORS12 = [0, 1, 3, 4, 5, 6, 8, 9, 10, 11]


def test_the_input_is_what_the_issue_asks_for():
    flags = [f for f, _ in INPUT12]
    assert len(INPUT12) == 12 and flags.count(U) == 2 and len(set(LABELS12)) == 4
    assert 1 in np.diff(CELLS12)                                        # a single-record cell
    assert LABELS12.index(b"ACGT") == 0 and LABELS12[2] == b"ACGT"      # a barcode that recurs
    assert LABELS12[1] == b"ACGT-1"                                      # ACGT next to ACGT-1, both ways
    assert P9[:8] == Q9[:8] and P9[8] != Q9[8] and LABELS12[3:] == [P9, Q9]
    assert INPUT12[7] == (U, b"\x00\xff") and INPUT12[6][1] != INPUT12[8][1]   # garbage on a cell boundary


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-o", EXE, SRC])
    return EXE


def test_streamed_cell_rule_equals_the_uncut_walk_for_every_cutting_under_sanitizers(exe):
    text = f"{len(INPUT12)}\n" + "".join(f"{f} {bc.hex() or '-'}\n" for f, bc in INPUT12)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    want = ("ok 2048 5 2 | " + " ".join(map(str, CELLS12)) + " | " + " ".join(b.hex() for b in LABELS12) + " | "
            + " ".join(map(str, SURVIVORS12)))
    assert r.stdout.strip() == want


def _collated(n_cells=4, per_cell=5):
    """a small barcode-collated input: records, names, secondary, cell_rec_off, one barcode per cell (one recurs)"""
    n = n_cells * per_cell
    rec = np.zeros(n, dtype=ALN_RECORD)
    rec["ref_id"] = np.arange(n) % T
    names = [b"r%d" % (i // 2) for i in range(n)]
    sec = (np.arange(n) % 2).astype(np.uint8)
    cro = np.arange(n_cells + 1, dtype=np.uint64) * per_cell
    bcs = synth.make_barcodes(n_cells - 1) + [synth.make_barcodes(1)[0]]
    from oarfish_amd.types import pack_read_names
    return rec, pack_read_names(names, n), sec, cro, bcs


def _join(batches):
    rec = np.concatenate([b[0] for b in batches])
    out = [rec]
    for k in (1, 2):
        blob = np.concatenate([b[k][0] for b in batches])
        lens = np.concatenate([np.diff(b[k][1].astype(np.int64)) for b in batches])
        out.append([blob.tobytes()[a:a + l] for a, l in zip(np.cumsum(lens) - lens, lens)])
    out.append(np.concatenate([b[3] for b in batches]))
    return out


def test_cut_cell_records_round_trips():
    rec, names, sec, cro, bcs = _collated()
    n = len(rec)
    raw = names[0].tobytes()
    want_names = [raw[int(names[1][i]):int(names[1][i + 1])] for i in range(n)]
    want_bc = [bcs[c] for c in range(len(bcs)) for _ in range(int(cro[c + 1] - cro[c]))]
    for cuts in [(), (0,), (n,), (5,), (7, 7), (13, 2), (0, 0, n, n), tuple(range(1, n))]:
        batches = synth.cut_cell_records(rec, names, sec, cro, bcs, cuts)
        assert len(batches) == len(cuts) + 1
        edges = [0] + sorted(cuts) + [n]
        assert [len(b[0]) for b in batches] == list(np.diff(edges))
        for b in batches:
            assert b[1][1][0] == 0 and b[2][1][0] == 0 and len(b[1][1]) == len(b[0]) + 1 == len(b[2][1]) and len(b[3]) == len(b[0])
        r, bc, nm, s = _join(batches)
        assert r.tobytes() == rec.tobytes() and bc == want_bc and nm == want_names and np.array_equal(s, sec)
    # sprinkled unmapped records: empty name, empty barcode, counted by the cuts; without them the input comes back
    batches = synth.cut_cell_records(rec, names, sec, cro, bcs, (1, 9, 9, 20), unmapped_every=3)
    r, bc, nm, s = _join(batches)
    un = (r["flags"] & U) != 0
    assert len(r) == n + (n + 2) // 3 and un.sum() == (n + 2) // 3 and un[0] and [len(b[0]) for b in batches] == [1, 8, 0, 11, len(r) - 20]
    assert all(not bc[i] and not nm[i] for i in np.flatnonzero(un))
    keep = np.flatnonzero(~un)
    assert r[keep].tobytes() == rec.tobytes() and [bc[i] for i in keep] == want_bc and [nm[i] for i in keep] == want_names
    assert np.array_equal(s[keep], sec)
    with pytest.raises(ValueError):
        synth.cut_cell_records(rec, names, sec, cro, bcs, (n + 1,))
    with pytest.raises(ValueError):
        synth.cut_cell_records(rec, names, sec, cro, bcs[:-1], ())
    assert "cut_cell_records" in oarfish_amd.__all__ and "quantify_single_cell_from_record_batches" in oarfish_amd.__all__


def test_declared_exported_by_both_libraries_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "oarfish_em.h")).read(), flags=re.S)
    n_args = {NEW[0]: 2, NEW[1]: 9, NEW[2]: 6, NEW[3]: 8}
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
        assert m, "include/oarfish_em.h does not declare " + name
        assert len(m.group(1).split(",")) == n_args[name]
        assert name in _lib.ABI_SYMBOLS
        assert len(getattr(_lib.lib(), name).argtypes) == n_args[name]
    for path in (_b.LIB_PATH, _b.TESTING_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert set(NEW) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, path
    assert "#define OEM_ABI_VERSION 2" in src and C.sizeof(_lib.CellsStreamOptsC) == 88   # the options are not touched
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in doc, "INTEGRATION.md does not name " + name
    rule = open(HDR).read()
    assert "Cells from a barcode-collated stream" in rule and "struct ParseCellsStream" in rule


def test_null_sessions_and_sessions_without_a_device():
    L = _lib.lib()
    t = C.c_uint64(77)
    off = np.zeros(1, dtype=np.uint64)
    assert L.oem_cells_stream_set_barcodes(None, 0) == _lib.OEM_ERR_ARG and b"NULL session" in L.oem_last_error()
    assert L.oem_cells_stream_push_barcodes(None, None, 0, None, off.ctypes.data, None, off.ctypes.data, None,
                                            C.byref(t)) == _lib.OEM_ERR_ARG and t.value == 77
    assert L.oem_cells_stream_barcodes_dims(None, None, None, None, None, None) == _lib.OEM_ERR_ARG
    assert L.oem_cells_stream_barcodes_copy(None, None, None, None, None, None, None, None) == _lib.OEM_ERR_ARG
    if _lib.device_count() > 0:
        return
    o = _lib.CellsStreamOptsC()
    o.n_txps, o.max_iter, o.conv_thresh = T, 100, 1e-3
    h = C.c_void_p(1)
    assert L.oem_cells_stream_create(C.byref(o), None, C.byref(h)) == _lib.OEM_ERR_NO_DEVICE and not h.value
    with pytest.raises(_lib.OemError) as ei:
        CellsStream(T, filters=FILTERS, txp_len=np.full(T, 2000, dtype=np.uint64), barcodes=True)
    assert ei.value.code == _lib.OEM_ERR_NO_DEVICE


def test_the_wrapper_checks_its_own_arguments():
    with pytest.raises(ValueError, match="filters"):
        CellsStream(T, barcodes=True)
    with pytest.raises(ValueError, match="mode"):
        CellsStream(T, filters=FILTERS, txp_len=np.full(T, 2000, dtype=np.uint64), barcodes=True, mode="sorted")
    # push_batch checks lengths before it touches the library: a closed handle comes first, so use an object without one
    cs = CellsStream.__new__(CellsStream)
    cs._h, cs._L = C.c_void_p(1), None
    rec = np.zeros(3, dtype=ALN_RECORD)
    three = [b"a", b"b", b"c"]
    with pytest.raises(ValueError, match="secondary"):
        cs.push_batch(rec, three, three, secondary=[0, 1])
    with pytest.raises(ValueError, match="barcodes"):
        cs.push_batch(rec, three[:2], three)
    with pytest.raises(ValueError, match="names"):
        cs.push_batch(rec, three, three[:2])
    cs._h = C.c_void_p()
