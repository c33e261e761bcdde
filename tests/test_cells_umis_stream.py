"""The UMI sessions, without a device: the ABI's shape, the argument and state errors that precede device use, the
wrapper's own checks, the cutters with ``umis=``, and -- under the sanitizers -- the per-group deduplication with
group-local indices joined over every partition of the cells into groups (tests/native/cells_umis_stream_main.cpp)."""
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
from oarfish_amd.single_cell import SingleCellArgs
from oarfish_amd.types import pack_read_names

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "cells_umis_stream_main.cpp")
EXE = os.path.join(HERE, "native", "cells_umis_stream_main")
HDR = os.path.join(ROOT, "oarfish_amd", "csrc", "oem_collate.h")
NEW = ["oem_cells_stream_set_umis", "oem_cells_stream_push_barcodes_umis", "oem_cells_stream_umis_copy"]
FILTERS = dict(five_prime_clip=2 ** 32 - 1, three_prime_clip=2 ** 62, score_threshold=0.95, min_aligned_fraction=0.5,
               min_aligned_len=50, which_strand=0, score_prob_denom=5.0)
T = 8
U = REC_UNMAPPED
P9, Q9 = b"AAAAAAAAC", b"AAAAAAAAG"
A, B, CC, D = b"AAAA", b"CC", b"ACGT-1", b"G"
G = b"\x00\xff"
# barcode, name, secondary, unmapped, UMI: the input of tests/test_cells_umis_stream_gpu.py
INPUT17 = [(A, b"r2", 0, 0, b"ACGT"), (A, b"r1", 0, 0, b"ACGT"), (A, b"r3", 0, 0, b"ACG"), (A, b"r4", 0, 0, b""), (A, b"r4", 1, 0, b"ACG"),
           (A, G, 1, 1, G), (A, b"r5", 0, 0, b"ACG"), (B, b"x", 0, 0, b"ACGT"), (B, b"y", 0, 0, P9), (B, b"z", 0, 0, Q9),
           (CC, b"p", 0, 0, b"TT"), (CC, b"q", 0, 0, b"TT"), (CC, b"q", 1, 0, b"TT"), (D, b"solo", 0, 0, b"TT"), (A, b"r9", 0, 0, b"ACGT"),
           (A, b"r0", 0, 0, b"ACG"), (b"", G, 0, 1, b"")]


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-o", EXE, SRC])
    return EXE


def test_per_group_dedup_joined_equals_the_whole_walk_for_every_partition_under_sanitizers(exe):
    text = f"{len(INPUT17)}\n" + "".join(f"{U if un else 0} {bc.hex() or '-'} {nm.hex() or '-'} {sec} {um.hex() or '-'}\n"
                                          for bc, nm, sec, un, um in INPUT17)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    lines = [ln.split(" | ") for ln in r.stdout.strip().splitlines()]
    assert [ln[0] for ln in lines] == ["ok streamed sort 16", "ok streamed adjacent 16", "ok any-order sort 8", "ok any-order adjacent 8"]
    nums = [[list(map(int, part.split())) for part in ln[1:]] for ln in lines]
    # the streamed rule, sorting: A comes back as a new cell with the same UMIs and nothing is merged; r1 (record 1) sorts
    # before r2 (record 0) and survives it; r4's empty primary UMI keeps it out; all of ACGT-1's reads are one class
    assert nums[0] == [[1, 2, 3, 4, 7, 8, 9, 10, 13, 15, 14], [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11], [0, 3, 6, 7, 8, 10], [0, 4, 7, 8, 9, 11],
                       [2, 0, 1, 0, 0]]
    # ... only cutting: the first read in input order survives
    assert nums[1][0] == [0, 2, 3, 4, 7, 8, 9, 10, 13, 14, 15] and nums[1][4] == [2, 0, 1, 0, 0]
    # the any-order rule: A is one cell, r0 (15) and r1 (1) sort first and survive the earlier records
    assert nums[2] == [[15, 1, 3, 4, 7, 8, 9, 10, 13], [0, 1, 2, 4, 5, 6, 7, 8, 9], [0, 3, 6, 7, 8], [0, 4, 7, 8, 9], [4, 0, 1, 0]]
    assert nums[3][0] == [0, 2, 3, 4, 7, 8, 9, 10, 13] and nums[3][4] == [4, 0, 1, 0]


def test_declared_exported_by_both_libraries_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "oarfish_em.h")).read(), flags=re.S)
    n_args = {NEW[0]: 1, NEW[1]: 11, NEW[2]: 2}
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
    assert re.search(r"#define OEM_CELLS_STREAM_INFO_UMI_DUP_READS\s+10u", src) and _lib.OEM_CELLS_STREAM_INFO_UMI_DUP_READS == 10
    assert re.search(r"#define OEM_CELLS_STREAM_INFO_UMI_DUP_RECORDS\s+11u", src) and _lib.OEM_CELLS_STREAM_INFO_UMI_DUP_RECORDS == 11
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in doc, "INTEGRATION.md does not name " + name
    rule = open(HDR).read()
    assert "UMIs in the sessions" in rule


def test_null_sessions_and_sessions_without_a_device():
    L = _lib.lib()
    t = C.c_uint64(77)
    off = np.zeros(1, dtype=np.uint64)
    assert L.oem_cells_stream_set_umis(None) == _lib.OEM_ERR_ARG and b"NULL session" in L.oem_last_error()
    assert L.oem_cells_stream_push_barcodes_umis(None, None, 0, None, off.ctypes.data, None, off.ctypes.data, None, None, off.ctypes.data,
                                                 C.byref(t)) == _lib.OEM_ERR_ARG and t.value == 77
    assert b"NULL session" in L.oem_last_error()
    assert L.oem_cells_stream_umis_copy(None, None) == _lib.OEM_ERR_ARG and b"NULL session" in L.oem_last_error()
    if _lib.device_count() > 0:
        return
    with pytest.raises(_lib.OemError) as ei:
        CellsStream(T, filters=FILTERS, txp_len=np.full(T, 2000, dtype=np.uint64), barcodes=True, umis=True)
    assert ei.value.code == _lib.OEM_ERR_NO_DEVICE
    with pytest.raises(_lib.OemError) as ei:
        CellsStream(T, filters=FILTERS, txp_len=np.full(T, 2000, dtype=np.uint64), barcodes=True, collated=False, umis=True)
    assert ei.value.code == _lib.OEM_ERR_NO_DEVICE


def test_the_wrapper_checks_its_own_arguments():
    with pytest.raises(ValueError, match="barcodes=True"):
        CellsStream(T, umis=True)
    with pytest.raises(ValueError, match="barcodes=True"):
        CellsStream(T, filters=FILTERS, txp_len=np.full(T, 2000, dtype=np.uint64), umis=True)
    assert SingleCellArgs(output="x").umis is False
    # push_batch checks before it touches the library: use an object without a handle behind it
    cs = CellsStream.__new__(CellsStream)
    cs._h, cs._L, cs._umis = C.c_void_p(1), None, True
    rec = np.zeros(3, dtype=ALN_RECORD)
    three = [b"a", b"b", b"c"]
    with pytest.raises(ValueError, match="umis"):
        cs.push_batch(rec, three, three, umis=three[:2])
    with pytest.raises(ValueError, match="umis"):
        cs.push_batch(rec, three, three, umis=(np.zeros(4, dtype=np.uint8), np.arange(3, dtype=np.uint64)))
    cs._umis = False
    with pytest.raises(ValueError, match="UMI session"):
        cs.push_batch(rec, three, three, umis=three)
    cs._h = C.c_void_p()


def _input(n_cells=4, per_cell=5):
    n = n_cells * per_cell
    rec = np.zeros(n, dtype=ALN_RECORD)
    rec["ref_id"] = np.arange(n) % T
    names = [b"r%d" % (i // 2) for i in range(n)]
    sec = (np.arange(n) % 2).astype(np.uint8)
    cro = np.arange(n_cells + 1, dtype=np.uint64) * per_cell
    bcs = synth.make_barcodes(n_cells - 1) + [synth.make_barcodes(1)[0]]
    umis = [b"" if i % 4 == 3 else b"ACGT"[:1 + i % 4] * (1 + i % 3) for i in range(n)]      # lengths 0 .. 9, some empty
    return rec, pack_read_names(names, n), sec, cro, bcs, umis


def _join(batches):
    out = [np.concatenate([b[0] for b in batches])]
    for k in (1, 2, 4):
        blob = np.concatenate([b[k][0] for b in batches])
        lens = np.concatenate([np.diff(b[k][1].astype(np.int64)) for b in batches])
        out.append([blob.tobytes()[a:a + l] for a, l in zip(np.cumsum(lens) - lens, lens)])
    out.append(np.concatenate([b[3] for b in batches]))
    return out


@pytest.mark.parametrize("cutter", ["cells", "interleaved"])
def test_the_cutters_round_trip_with_umis(cutter):
    rec, names, sec, cro, bcs, umis = _input()
    n = len(rec)
    raw = names[0].tobytes()
    want_names = [raw[int(names[1][i]):int(names[1][i + 1])] for i in range(n)]
    want_bc = [bcs[c].encode() if isinstance(bcs[c], str) else bcs[c] for c in range(len(bcs)) for _ in range(int(cro[c + 1] - cro[c]))]
    upair = pack_read_names(umis, n)

    def cut(cuts, with_umis=True, **kw):
        kw = dict(kw, umis=upair) if with_umis else kw
        if cutter == "cells":
            return synth.cut_cell_records(rec, names, sec, cro, bcs, cuts, **kw)
        return synth.cut_interleaved_records(rec, names, sec, pack_read_names(want_bc, n), cuts, **kw)

    for cuts in [(), (0,), (n,), (5,), (7, 7), (13, 2), tuple(range(1, n))]:
        batches = cut(cuts)
        assert len(batches) == len(cuts) + 1 and all(len(b) == 5 for b in batches)
        for b in batches:
            assert b[4][1][0] == 0 and len(b[4][1]) == len(b[0]) + 1 and b[4][1].dtype == np.uint64 and int(b[4][1][-1]) == len(b[4][0])
        r, bc, nm, um, s = _join(batches)
        assert r.tobytes() == rec.tobytes() and bc == want_bc and nm == want_names and um == umis and np.array_equal(s, sec)
        plain = cut(cuts, with_umis=False)                                   # without umis nothing changes
        assert all(len(p) == 4 for p in plain)
        for p, b in zip(plain, batches):
            assert p[0].tobytes() == b[0].tobytes() and all(np.array_equal(p[k][j], b[k][j]) for k in (1, 2) for j in (0, 1))
    batches = cut((1, 9, 9, 20), unmapped_every=3)                           # sprinkled records have empty UMIs
    r, bc, nm, um, s = _join(batches)
    un = (r["flags"] & U) != 0
    assert len(r) == n + (n + 2) // 3 and un.sum() == (n + 2) // 3 and un[0]
    assert all(not um[i] and not bc[i] and not nm[i] for i in np.flatnonzero(un))
    keep = np.flatnonzero(~un)
    assert r[keep].tobytes() == rec.tobytes() and [um[i] for i in keep] == umis and [nm[i] for i in keep] == want_names
    with pytest.raises(ValueError, match="umis"):
        cut((), with_umis=False, umis=pack_read_names(umis[:-1], n - 1))


def test_recollate_by_first_barcode_is_stable():
    bcs = [b"T", b"A", b"T", b"GG", b"A", b"T", b"GG"]
    perm = synth.recollate_by_first_barcode(pack_read_names(bcs, len(bcs)))
    assert list(perm) == [0, 2, 5, 1, 4, 3, 6]
    assert len(synth.recollate_by_first_barcode(pack_read_names([], 0))) == 0
    assert "recollate_by_first_barcode" in dir(oarfish_amd.synth)
