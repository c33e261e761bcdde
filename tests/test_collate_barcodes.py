"""CPU tests of the barcode collation (oem_collate_barcodes, oem_em_run_cells_records_barcodes_sparse): declared, exported
by both libraries, bound with the header's argument counts, every host-visible argument error before any device use, the
Python wrapper's own checks, the synthetic inputs, and the host walk of the barcode rule
(oarfish_amd/csrc/oem_collate.h, collate_barcodes_host) in a stand-alone program under the address and
undefined-behaviour sanitizers.

The oracle is NumPy and knows nothing of the C++ walk: a stable argsort by barcode bytes (``bytes`` compare unsigned and
lexicographic, a proper prefix first), the runs of one barcode ranked by their first record.
tests/test_collate_barcodes_gpu.py holds the device to the same oracle on the same cases."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth, writers
from oarfish_amd import build as _b
from oarfish_amd.builder import ALN_RECORD, filters_c
from tests.test_collate import ADJACENT, SORT, pack

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "collate_barcodes_main.cpp")
EXE = os.path.join(HERE, "native", "collate_barcodes_main")
HDR = os.path.join(ROOT, "oarfish_amd", "csrc", "oem_collate.h")
COLLATE = "oem_collate_barcodes"
ONE_CALL = "oem_em_run_cells_records_barcodes_sparse"
T = 40
FILTERS = dict(five_prime_clip=2 ** 32 - 1, three_prime_clip=2 ** 62, score_threshold=0.95, min_aligned_fraction=0.5,
               min_aligned_len=50, which_strand=0, score_prob_denom=5.0)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
def oracle(barcodes):
    """(order, cell_rec_off) as lists; barcodes: a list of bytes, one per record."""
    n = len(barcodes)
    rank = {b: k for k, b in enumerate(sorted(set(barcodes)))}           # bytes: unsigned, lexicographic, prefix first
    by_bytes = np.argsort(np.array([rank[b] for b in barcodes], dtype=np.int64), kind="stable")
    runs, heads = [], []
    for p, i in enumerate(by_bytes):
        if p == 0 or barcodes[i] != barcodes[by_bytes[p - 1]]:
            runs.append([])
            heads.append(int(i))                                         # a run's first record is its smallest
        runs[-1].append(int(i))
    order, cro = [], [0]
    for r in np.argsort(np.array(heads, dtype=np.int64), kind="stable"):  # first seen first
        order += runs[r]
        cro.append(len(order))
    assert len(order) == n
    return order, cro


def barcode_cases():
    """name -> the records' barcodes."""
    base = bytes(range(0x41, 0x41 + 26))
    rng = np.random.default_rng(5)
    cases = {}
    for at in (7, 8, 15):     # the last byte of key 0, the first of key 1, the last of key 1
        a, b = bytearray(base[:18]), bytearray(base[:18])
        a[at], b[at] = 0x7a, 0x79
        cases[f"differ_in_byte_{at}"] = [bytes(a), bytes(b), bytes(a), bytes(b), bytes(b), bytes(a)]
    cases["prefix"] = [b"ACGTACGTAC", b"ACGT", b"ACGTACGT", b"ACGT", b"ACGTACGTAC", b"ACGTACGTA", b"ACGTACGT"]
    lens = [base[:n] for n in (1, 8, 9, 16)]
    cases["lengths"] = [lens[i] for i in rng.integers(0, 4, size=40)]
    cases["one_cell"] = [b"ACGTACGTACGTACGT-1"] * 9
    cases["every_record_its_own_cell"] = [b"bc%03d" % ((i * 37) % 101) for i in range(101)]
    cases["one_record"] = [b"A"]
    cases["no_records"] = []
    hi = [bytes([v]) + b"t" for v in (0x80, 0x7f, 0xff, 0x01)] + [b"abcdefg" + bytes([v]) for v in (0x80, 0x7f, 0xff)] \
        + [b"abcdefgh" + bytes([v]) for v in (0xfe, 0x7e, 0x80)]
    cases["unsigned"] = [hi[i] for i in rng.integers(0, len(hi), size=60)]
    cases["interleaved_10x"] = [synth.make_barcodes(9, "10x")[i] for i in rng.integers(0, 9, size=200)]
    cases["interleaved_var"] = [synth.make_barcodes(30, "var")[i] for i in rng.integers(0, 30, size=300)]
    return cases


def test_the_oracle_itself():
    assert oracle([b"b", b"a", b"b", b"c", b"a"]) == ([0, 2, 1, 4, 3], [0, 2, 4, 5])               # first seen: b, a, c
    assert oracle([b"AC", b"A", b"AC", b"A"]) == ([0, 2, 1, 3], [0, 2, 4])
    assert oracle([]) == ([], [0])
    assert oracle([bytes([0xff]), bytes([0x01]), bytes([0xff])]) == ([0, 2, 1], [0, 2, 3])
    order, cro = oracle([b"x"] * 3 + [b"y"] * 2)                       # collated input: the identity, today's cells
    assert order == list(range(5)) and cro == [0, 3, 5]


# ---------------------------------------------------------------------------------------------------------------------
# declared, exported, bound
# ---------------------------------------------------------------------------------------------------------------------
def _declaration(name):
    src = open(os.path.join(ROOT, "include", "oarfish_em.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
    assert m, "include/oarfish_em.h does not declare " + name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,n_args,first,last", [(COLLATE, 7, "const uint8_t *barcodes", "uint64_t *out_n_cells"),
                                                    (ONE_CALL, 25, "const oem_filters *filters", "oem_cells_result **out")])
def test_declared_exported_by_both_libraries_and_bound(name, n_args, first, last):
    args = _declaration(name)
    assert len(args) == n_args and args[0] == first and args[-1] == last
    for path in (_b.LIB_PATH, _b.TESTING_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert name in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, path
    assert name in _lib.ABI_SYMBOLS
    assert len(getattr(_lib.lib(), name).argtypes) == n_args
    assert len(getattr(_lib.testing_lib(), name).argtypes) == n_args
    assert _lib.lib().oem_abi_version() == 2
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = [ln for ln in doc.splitlines() if name in ln and ln.lstrip().startswith("|")]
    assert row and "single_cell.rs:196-213" in row[0] and "alignment_parser.rs:244-299" in row[0], "INTEGRATION.md has no row for it"


# ---------------------------------------------------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------------------------------------------------
def _collate_input():
    blob, off = pack([b"AC", b"G", b"AC", b"TTT", b"G"])
    return dict(blob=blob, off=off, n=5)


def _collate_call(L, blob, off, n, outs=(True, True, True)):
    order = np.zeros(max(n, 1) if n < 2 ** 20 else 1, dtype=np.uint32)
    cro = np.zeros((n if n < 2 ** 20 else 0) + 1, dtype=np.uint64)
    nc = C.c_uint64(0)
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    rc = L.oem_collate_barcodes(ptr(blob), ptr(off), n, 0, order.ctypes.data if outs[0] else None, cro.ctypes.data if outs[1] else None,
                                C.byref(nc) if outs[2] else None)
    return rc, L.oem_last_error() or b"", (order, cro, int(nc.value))


def test_collate_argument_errors_come_before_any_device_use():
    L = _lib.lib()
    a = _collate_input()
    off_from_1 = a["off"].copy()
    off_from_1[0] = 1
    off_dec = a["off"].copy()
    off_dec[2] = 1
    cases = [   # (what is wrong, arguments, a word of the message)
        ("barcodes NULL", dict(blob=None), b"barcodes is NULL"),
        ("barcode_off NULL", dict(off=None), b"NULL"),
        ("barcode_off not from 0", dict(off=off_from_1), b"barcode_off must start at 0"),
        ("barcode_off decreases", dict(off=off_dec), b"barcode_off must be non-decreasing (record 1)"),
        ("too many records", dict(n=2 ** 32), b"2^32 - 1"),
    ]
    for what, kw, word in cases:
        b = dict(a)
        b.update(kw)
        rc, msg, _ = _collate_call(L, **b)
        assert rc == _lib.OEM_ERR_ARG, (what, rc, msg)
        assert word in msg and COLLATE.encode() in msg, (what, msg)
    for k in range(3):
        rc, msg, _ = _collate_call(L, **a, outs=tuple(j != k for j in range(3)))
        assert rc == _lib.OEM_ERR_ARG and b"NULL" in msg and COLLATE.encode() in msg, (k, rc, msg)


def _input():
    """Five records of three barcodes, interleaved."""
    rec = np.zeros(5, dtype=ALN_RECORD)
    for i in range(5):
        rec[i] = (i % T, 10, 1500, 1400, 1000 - i, 1500, _lib.REC_HAS_SCORE, 0)
    blob, off = pack([b"r2", b"r1", b"r2", b"q", b"q"])
    bc_blob, bc_off = pack([b"AC", b"G", b"AC", b"TTT", b"G"])
    return dict(F=filters_c(FILTERS), tl=np.full(T, 2000, dtype=np.uint64), rec=rec, bc_blob=bc_blob, bc_off=bc_off, blob=blob, off=off,
                sec=np.array([0, 0, 1, 0, 1], dtype=np.uint8))


def _call(L, F, tl, rec, bc_blob, bc_off, blob, off, sec, n_txps=T, n=5, mode=SORT, bin_width=100, model=-1, out=True):
    res = C.c_void_p(1)
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    rc = getattr(L, ONE_CALL)(None if F is None else C.addressof(F), ptr(tl), n_txps, ptr(rec), n, ptr(bc_blob), ptr(bc_off), ptr(blob),
                              ptr(off), ptr(sec), mode, bin_width, model, 2.0, 0, 100, 1e-3, None, None, None, None, None, None, None,
                              C.byref(res) if out else None)
    return rc, res, L.oem_last_error() or b""


def test_one_call_argument_errors_come_before_any_device_use():
    L = _lib.lib()
    a = _input()

    def moved(off, at, v):
        off = off.copy()
        off[at] = v
        return off

    cases = [   # (what is wrong, arguments, a word of the message): the records call's, the barcodes', the names'
        ("filters NULL", dict(F=None), b"bad argument"),
        ("txp_len NULL", dict(tl=None), b"bad argument"),
        ("n_txps 0", dict(n_txps=0), b"bad argument"),
        ("model 2", dict(model=2), b"model"),
        ("model -2", dict(model=-2), b"model"),
        ("bin width 0 with a model", dict(model=1, bin_width=0), b"bin width"),
        ("records NULL", dict(rec=None), b"records is NULL"),
        ("barcodes NULL", dict(bc_blob=None), b"barcodes is NULL"),
        ("barcode_off NULL", dict(bc_off=None), b"NULL"),
        ("barcode_off not from 0", dict(bc_off=moved(a["bc_off"], 0, 1)), b"barcode_off must start at 0"),
        ("barcode_off decreases", dict(bc_off=moved(a["bc_off"], 2, 1)), b"barcode_off must be non-decreasing (record 1)"),
        ("names NULL", dict(blob=None), b"names is NULL"),
        ("name_off NULL", dict(off=None), b"NULL"),
        ("name_off not from 0", dict(off=moved(a["off"], 0, 1)), b"name_off must start at 0"),
        ("name_off decreases", dict(off=moved(a["off"], 2, 1)), b"name_off must be non-decreasing (record 1)"),
        ("too many records", dict(n=2 ** 32), b"2^32 - 1"),
        ("no such mode", dict(mode=2), b"mode"),
    ]
    for what, kw, word in cases:
        b = dict(a)
        b.update(kw)
        rc, res, msg = _call(L, **b)
        assert rc == _lib.OEM_ERR_ARG, (what, rc, msg)
        assert not res.value, what
        assert word in msg and ONE_CALL.encode() in msg or word == b"bin width" and word in msg, (what, msg)
    rc, _, msg = _call(L, **a, out=False)
    assert rc == _lib.OEM_ERR_ARG and b"out is NULL" in msg


def test_well_formed_input_needs_a_device():
    L = _lib.lib()
    rc, msg, got = _collate_call(L, **_collate_input())
    if _lib.device_count() > 0:
        assert rc == _lib.OEM_OK, msg
        assert (list(got[0]), list(got[1][:got[2] + 1])) == oracle([b"AC", b"G", b"AC", b"TTT", b"G"])
    else:
        assert rc == _lib.OEM_ERR_NO_DEVICE, (rc, msg)
        with pytest.raises(_lib.OemError) as e:
            oarfish_amd.collate_barcodes([b"AC", b"G", b"AC"])
        assert e.value.code == _lib.OEM_ERR_NO_DEVICE
    a = _input()
    for mode in (SORT, ADJACENT):
        for model in (-1, 0, 1):
            rc, res, msg = _call(L, **a, mode=mode, model=model)
            if _lib.device_count() > 0:
                assert rc == _lib.OEM_OK and res.value, msg
                L.oem_cells_result_destroy(res)
            else:
                assert rc == _lib.OEM_ERR_NO_DEVICE and not res.value, (rc, msg)
    if _lib.device_count() == 0:
        for collate in ("host", "device"):
            with pytest.raises(oarfish_amd.OemError) as e:
                oarfish_amd.em_cells_records_sparse(FILTERS, a["tl"], a["rec"], None, None, names=(a["blob"], a["off"]), secondary=a["sec"],
                                                    barcodes=(a["bc_blob"], a["bc_off"]), collate=collate)
            assert e.value.code == _lib.OEM_ERR_NO_DEVICE


def test_the_wrapper_checks_its_own_arguments():
    a = _input()
    names, barcodes = (a["blob"], a["off"]), (a["bc_blob"], a["bc_off"])
    run = lambda *p, **kw: oarfish_amd.em_cells_records_sparse(FILTERS, a["tl"], *p, **kw)   # noqa: E731
    cro = np.array([0, 2, 4, 5], dtype=np.uint64)
    for collate in ("host", "device"):
        with pytest.raises(ValueError, match="cell_group_off must be None"):
            run(a["rec"], None, cro, names=names, barcodes=barcodes, collate=collate)
        with pytest.raises(ValueError, match="cell_group_off must be None"):
            run(a["rec"], cro, None, names=names, barcodes=barcodes, collate=collate)
        with pytest.raises(ValueError, match="needs names"):
            run(a["rec"], None, None, barcodes=barcodes, collate=collate)
        with pytest.raises(ValueError, match="names must have one entry per record"):
            run(a["rec"][:4], None, None, names=names, barcodes=barcodes, collate=collate)
        with pytest.raises(ValueError, match="barcodes must have one entry per record"):
            run(a["rec"], None, None, names=names, barcodes=[b"A"] * 4, collate=collate)
        with pytest.raises(ValueError, match="secondary must have one entry per record"):
            run(a["rec"], None, None, names=names, barcodes=barcodes, secondary=a["sec"][:4], collate=collate)
    for bad in ("gpu", "", None):
        with pytest.raises(ValueError, match="collate"):
            run(a["rec"], None, None, names=names, barcodes=barcodes, collate=bad)
    with pytest.raises(ValueError, match="mode"):
        run(a["rec"], None, None, names=names, barcodes=barcodes, collate="device", mode="sorted")


# ---------------------------------------------------------------------------------------------------------------------
# the synthetic inputs and the writer's helper
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style", ["10x", "var"])
def test_make_barcodes_gives_distinct_barcodes(style):
    b = synth.make_barcodes(200, style, seed=3)
    assert len(b) == 200 and len(set(b)) == 200 and all(isinstance(x, bytes) and x and 0 not in x for x in b)
    assert b == synth.make_barcodes(200, style, seed=3) and b != synth.make_barcodes(200, style, seed=4)
    if style == "10x":
        assert all(len(x) == 18 and x.endswith(b"-1") for x in b)
    else:
        assert {len(x) for x in b} >= {1, 8, 9, 16, 20} and max(len(x) for x in b) == 20
        assert sum(any(y != x and y.startswith(x) for y in b) for x in b) >= 20     # proper prefixes of other barcodes
    with pytest.raises(ValueError):
        synth.make_barcodes(3, "11x")


@pytest.mark.parametrize("how", ["uniform", "blocks"])
def test_interleave_cells_is_a_permutation_of_its_input(how):
    cro = np.array([0, 30, 31, 31, 90, 200], dtype=np.uint64)
    n = 200
    rng = np.random.default_rng(1)
    names_list = [b"n%d" % v * int(rng.integers(1, 4)) for v in rng.integers(0, 50, size=n)]
    rec = np.zeros(n, dtype=ALN_RECORD)
    rec["ref_id"] = np.arange(n)
    sec = rng.integers(0, 2, size=n).astype(np.uint8)
    barcodes = synth.make_barcodes(5, "var", seed=2)
    r2, (blob, off), s2, (bc_blob, bc_off), perm = synth.interleave_cells(rec, pack(names_list), sec, cro, barcodes, seed=9, how=how)
    assert sorted(perm.tolist()) == list(range(n)) and perm.tolist() != list(range(n))
    assert np.array_equal(r2["ref_id"], perm) and np.array_equal(s2, sec[perm])
    cell_of = np.repeat(np.arange(5), np.diff(cro.astype(np.int64)))
    for k in range(n):
        assert bytes(blob[int(off[k]):int(off[k + 1])]) == names_list[perm[k]]
        assert bytes(bc_blob[int(bc_off[k]):int(bc_off[k + 1])]) == barcodes[cell_of[perm[k]]]
    if how == "blocks":     # runs of a few records of one cell
        assert 1.5 < n / (1 + int((np.diff(perm) != 1).sum())) < 8
    with pytest.raises(ValueError):
        synth.interleave_cells(rec, pack(names_list), sec, cro, barcodes, how="sorted")
    # the oracle finds the cells again, first seen first; the helper names them
    per_record = [bytes(bc_blob[int(bc_off[k]):int(bc_off[k + 1])]) for k in range(n)]
    order, cell_rec_off = oracle(per_record)
    got = writers.cell_barcodes((bc_blob, bc_off), order, cell_rec_off)
    first_seen = list(dict.fromkeys(per_record))
    assert got == [b.decode() for b in first_seen] and len(got) == 4            # (one cell of the five has no record)
    assert writers.cell_barcodes(per_record, order, cell_rec_off) == got


# ---------------------------------------------------------------------------------------------------------------------
# oem_collate.h's barcode rule, stand-alone, under sanitizers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-o", EXE, SRC])
    return EXE


def _request(barcodes):
    return "\n".join([f"B {len(barcodes)}"] + [b.hex() or "-" for b in barcodes]) + "\n"


def _walk(exe, requests):
    r = subprocess.run([exe], input="".join(requests), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[-1] == "" and len(out) == len(requests) + 1
    return out[:-1]


def _parse(line):
    head, order, cro = line.split("|")
    assert head.split()[0] == "ok"
    return int(head.split()[1]), [int(x) for x in order.split()], [int(x) for x in cro.split()]


def test_host_walk_matches_the_oracle_under_sanitizers(exe):
    cases = barcode_cases()
    answers = _walk(exe, [_request(v) for v in cases.values()])
    for (name, barcodes), line in zip(cases.items(), answers):
        order, cro = oracle(barcodes)
        assert _parse(line) == (len(cro) - 1, order, cro), name


def bad_barcode_cases():
    """(barcodes, the first bad record, whether it is a 0 byte): empty and 0 byte, first, middle and last."""
    good = [b"ACGTACGTAC%02d" % (i % 7) for i in range(40)]
    out = []
    for at in (0, 17, 39):
        for bad, zero in ((b"", 0), (b"ACGTACGT\x00C", 1), (b"\x00", 1)):
            b = list(good)
            b[at] = bad
            if at == 17:
                b[30] = b"" if zero else b"A\x00"     # a later bad one of the other kind does not win
            out.append((b, at, zero))
    return out


def test_host_walk_reports_the_first_bad_barcode(exe):
    cases = bad_barcode_cases()
    assert _walk(exe, [_request(b) for b, _, _ in cases]) == [f"bad {at} {zero}" for _, at, zero in cases]
