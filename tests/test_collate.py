"""CPU tests of the name collation (oem_collate_names): declared, exported by both libraries, bound with the header's
argument count, every host-visible argument error before any device use, and the host walk of the rule
(oarfish_amd/csrc/oem_collate.h) in a stand-alone program under the address and undefined-behaviour sanitizers, held to
the oracle below.

The oracle is pure Python and knows nothing of the C++ walk: per cell ``sorted`` over (name bytes, secondary, index) --
``bytes`` compare unsigned and lexicographic with a proper prefix first, as ``<[u8]>::cmp`` does -- and a group cut
wherever the bytes change.  tests/test_collate_gpu.py holds the device to the same oracle on the same cases."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oarfish_amd import _lib
from oarfish_amd import build as _b

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "collate_main.cpp")
EXE = os.path.join(HERE, "native", "collate_main")
HDR = os.path.join(ROOT, "oarfish_amd", "csrc", "oem_collate.h")
SORT, ADJACENT = 0, 1


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
def oracle(names, sec, cell_rec_off, mode=SORT):
    """(order, group_off, cell_group_off) as lists; names: a list of bytes, sec: a list of flags or None."""
    order, group_off, cell_group_off = [], [], []
    for c in range(len(cell_rec_off) - 1):
        a, b = int(cell_rec_off[c]), int(cell_rec_off[c + 1])
        idx = list(range(a, b))
        if mode == SORT:
            idx = sorted(idx, key=lambda i: (names[i], bool(sec[i]) if sec is not None else False, i))
        cell_group_off.append(len(group_off))
        for k, i in enumerate(idx):
            if k == 0 or names[i] != names[idx[k - 1]]:
                group_off.append(a + k)
        order += idx
    cell_group_off.append(len(group_off))
    group_off.append(len(names))
    return order, group_off, cell_group_off


def pack(names):
    blob = np.frombuffer(b"".join(names), dtype=np.uint8).copy()
    off = np.zeros(len(names) + 1, dtype=np.uint64)
    np.cumsum([len(n) for n in names], out=off[1:])
    return blob, off


# ---------------------------------------------------------------------------------------------------------------------
# the cases both tiers run: name -> (names, secondary or None, cell_rec_off)
# ---------------------------------------------------------------------------------------------------------------------
def _scramble(names, sec, seed):
    perm = np.random.default_rng(seed).permutation(len(names))
    return [names[i] for i in perm], None if sec is None else [sec[i] for i in perm]


def fixture_cases():
    cases = {}
    base = bytes(range(0x41, 0x41 + 26)) * 10
    # key edges, one cell: the lengths around the 8-byte keys
    lens = [1, 7, 8, 9, 15, 16, 17, 24, 25, 255]
    names = [base[:n] for n in lens] + [b"Q" + base[:n - 1] for n in lens]
    cases["lengths"] = (*_scramble(names, None, 1), [0, len(names)])
    # equal through 8, 16 and 24 bytes, different in the next one (and one that ends there)
    names = []
    for n in (8, 16, 24):
        names += [base[:n] + b"x", base[:n] + b"y", base[:n] + b"xz", base[:n]]
    cases["shared_keys"] = (*_scramble(names, None, 2), [0, len(names)])
    cases["prefix"] = ([b"r10", b"r1/2", b"r1", b"r10", b"r1"], None, [0, 5])
    # unsigned comparison at a deciding byte: first byte, last byte of a key, first byte of the second key
    names = []
    for lead in (b"", b"abcdefg", b"abcdefgh"):
        names += [lead + bytes([v]) + b"t" for v in (0x80, 0x7f, 0xff, 0x01, 0x80)]
    cases["unsigned"] = (*_scramble(names, None, 3), [0, len(names)])
    # ties
    cases["one_read_scrambled"] = ([b"read-one"] * 4 + [b"other"], [1, 1, 0, 1, 0], [0, 5])
    cases["two_primaries"] = ([b"b", b"a", b"b", b"a", b"b"], [0, 0, 1, 0, 0], [0, 5])
    cases["secondary_null"] = ([b"b", b"a", b"b", b"a", b"b"], None, [0, 5])
    cases["long_tie"] = ([base[:40]] * 3 + [base[:39]] * 2, [1, 0, 1, 1, 0], [0, 5])
    # cells
    cases["empty_cells"] = ([b"n2", b"n1", b"n2", b"n9", b"n1"], [0, 0, 1, 0, 1], [0, 0, 3, 3, 5, 5])
    cases["one_record_cells"] = ([b"solo", b"z", b"a", b"solo"], None, [0, 1, 3, 4])
    cases["same_name_adjacent_cells"] = ([b"rr", b"rr", b"aa", b"rr", b"rr"], [0, 1, 0, 1, 0], [0, 2, 5])
    cases["no_records"] = ([], None, [0, 0, 0])
    cases["no_cells"] = ([], None, [0])
    return cases


def adjacent_cases():
    sorted_names = [b"a", b"a", b"b", b"c", b"c", b"c", b"a", b"d"]
    return {
        "name_sorted": (sorted_names, [0, 1, 0, 0, 1, 1, 0, 0], [0, 6, 8]),
        "recurs": ([b"x", b"y", b"x", b"x", b"abcdefgh1", b"abcdefgh2", b"abcdefgh2"], None, [0, 7]),
        "cell_ends_inside_a_name": ([b"k", b"k", b"k"], None, [0, 2, 2, 3]),
    }


# ---------------------------------------------------------------------------------------------------------------------
# declared, exported, bound
# ---------------------------------------------------------------------------------------------------------------------
def _declaration():
    src = open(os.path.join(ROOT, "include", "oarfish_em.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+oem_collate_names\s*\(([^;]*)\)\s*;", src)
    assert m, "include/oarfish_em.h does not declare oem_collate_names"
    return [a.strip() for a in m.group(1).split(",")]


def test_declared_exported_by_both_libraries_and_bound():
    args = _declaration()
    assert len(args) == 12 and args[0].startswith("const uint8_t *names") and args[-1].endswith("out_cell_group_off")
    for path in (_b.LIB_PATH, _b.TESTING_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert "oem_collate_names" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, path
    assert "oem_collate_names" in _lib.ABI_SYMBOLS
    assert len(_lib.lib().oem_collate_names.argtypes) == len(args)
    assert len(_lib.testing_lib().oem_collate_names.argtypes) == len(args)
    hdr = open(os.path.join(ROOT, "include", "oarfish_em.h")).read()
    assert "#define OEM_COLLATE_SORT 0u" in hdr and "#define OEM_COLLATE_ADJACENT 1u" in hdr
    assert (_lib.OEM_COLLATE_SORT, _lib.OEM_COLLATE_ADJACENT) == (0, 1)


def test_integration_doc_maps_it_to_the_reference():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = [ln for ln in doc.splitlines() if "oem_collate_names" in ln and ln.lstrip().startswith("|")]
    assert row and "alignment_parser.rs:170-241" in row[0] and ":301-437" in row[0]


# ---------------------------------------------------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------------------------------------------------
def _input():
    names = [b"r2", b"r1", b"r2", b"q", b"q"]
    blob, off = pack(names)
    return dict(blob=blob, off=off, sec=np.array([0, 0, 1, 0, 1], dtype=np.uint8), n=5, cro=np.array([0, 3, 3, 5], dtype=np.uint64),
                n_cells=3, mode=SORT)


def _call(L, blob, off, sec, n, cro, n_cells, mode, outs=(True, True, True, True)):
    order = np.zeros(max(n, 1) if n < 2 ** 20 else 1, dtype=np.uint32)
    goff = np.zeros((n if n < 2 ** 20 else 0) + 1, dtype=np.uint64)
    cgo = np.zeros(n_cells + 1, dtype=np.uint64)
    ng = C.c_uint64(0)
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    rc = L.oem_collate_names(ptr(blob), ptr(off), ptr(sec), n, ptr(cro), n_cells, mode, 0,
                             order.ctypes.data if outs[0] else None, goff.ctypes.data if outs[1] else None,
                             C.byref(ng) if outs[2] else None, cgo.ctypes.data if outs[3] else None)
    return rc, L.oem_last_error() or b"", (order, goff, int(ng.value), cgo)


def test_argument_errors_come_before_any_device_use():
    L = _lib.lib()
    a = _input()
    off_from_1 = a["off"].copy()
    off_from_1[0] = 1
    off_dec = a["off"].copy()
    off_dec[2] = 1
    cases = [   # (what is wrong, arguments, a word of the message)
        ("names NULL", dict(blob=None), b"names is NULL"),
        ("name_off NULL", dict(off=None), b"NULL"),
        ("cell_rec_off NULL", dict(cro=None), b"NULL"),
        ("name_off not from 0", dict(off=off_from_1), b"name_off must start at 0"),
        ("name_off decreases", dict(off=off_dec), b"name_off must be non-decreasing (record 1)"),
        ("cell_rec_off not from 0", dict(cro=np.array([1, 3, 3, 5], dtype=np.uint64)), b"cell_rec_off must start at 0"),
        ("cell_rec_off decreases", dict(cro=np.array([0, 4, 3, 5], dtype=np.uint64)), b"cell_rec_off must be non-decreasing (cell 1)"),
        ("cell_rec_off short of n_records", dict(cro=np.array([0, 3, 3, 4], dtype=np.uint64)), b"n_records"),
        ("cell_rec_off past n_records", dict(cro=np.array([0, 3, 3, 6], dtype=np.uint64)), b"n_records"),
        ("too many records", dict(n=2 ** 32), b"2^32 - 1"),
        ("no such mode", dict(mode=2), b"mode"),
    ]
    for what, kw, word in cases:
        b = dict(a)
        b.update(kw)
        rc, msg, _ = _call(L, **b)
        assert rc == _lib.OEM_ERR_ARG, (what, rc, msg)
        assert word in msg and b"oem_collate_names" in msg, (what, msg)
    for k in range(4):
        outs = tuple(j != k for j in range(4))
        rc, msg, _ = _call(L, **a, outs=outs)
        assert rc == _lib.OEM_ERR_ARG and b"NULL" in msg, (k, rc, msg)


def test_well_formed_input_needs_a_device():
    import oarfish_amd
    a = _input()
    rc, msg, got = _call(_lib.lib(), **a)
    names = [b"r2", b"r1", b"r2", b"q", b"q"]
    if _lib.device_count() > 0:
        assert rc == _lib.OEM_OK, msg
        want = oracle(names, [0, 0, 1, 0, 1], [0, 3, 3, 5])
        assert (list(got[0]), list(got[1][:got[2] + 1]), list(got[3])) == want
    else:
        assert rc == _lib.OEM_ERR_NO_DEVICE, (rc, msg)
        with pytest.raises(_lib.OemError) as e:
            oarfish_amd.collate_names(names, [0, 3, 3, 5], [0, 0, 1, 0, 1])
        assert e.value.code == _lib.OEM_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        oarfish_amd.collate_names(names, [0, 5], mode="sorted")
    with pytest.raises(ValueError):
        oarfish_amd.collate_names(names, [0, 5], secondary=[0, 1])


# ---------------------------------------------------------------------------------------------------------------------
# oem_collate.h, stand-alone, under sanitizers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-o", EXE, SRC])
    return EXE


def _request(names, sec, cro, mode):
    lines = [f"C {mode} {len(names)} {len(cro) - 1} {0 if sec is None else 1}", " ".join(str(int(x)) for x in cro)]
    for i, n in enumerate(names):
        lines.append(f"{n.hex() or '-'} {0 if sec is None else int(sec[i])}")
    return "\n".join(lines) + "\n"


def _walk(exe, requests):
    r = subprocess.run([exe], input="".join(requests), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[-1] == "" and len(out) == len(requests) + 1
    return out[:-1]


def _parse(line):
    head, order, goff, cgo = line.split("|")
    assert head.split()[0] == "ok"
    return int(head.split()[1]), [int(x) for x in order.split()], [int(x) for x in goff.split()], [int(x) for x in cgo.split()]


def test_host_walk_matches_the_oracle_under_sanitizers(exe):
    todo = [(k, v, SORT) for k, v in fixture_cases().items()]
    todo += [(k, v, ADJACENT) for k, v in fixture_cases().items()]
    todo += [(k, v, ADJACENT) for k, v in adjacent_cases().items()]
    rng = np.random.default_rng(11)
    for k in range(3):   # random short names over a small alphabet: many ties and prefixes
        n = 300
        names = [bytes(rng.integers(0x61, 0x64, size=int(rng.integers(1, 12))).astype(np.uint8)) for _ in range(n)]
        sec = [int(x) for x in rng.integers(0, 2, size=n)]
        todo.append((f"random{k}", (names, sec, [0, 100, 100, 290, 300]), SORT))
    answers = _walk(exe, [_request(*v, mode) for _, v, mode in todo])
    for (name, (names, sec, cro), mode), line in zip(todo, answers):
        order, goff, cgo = oracle(names, sec, cro, mode)
        assert _parse(line) == (len(goff) - 1, order, goff, cgo), (name, mode)


def test_host_walk_reports_the_first_bad_name(exe):
    answers = _walk(exe, [_request([b"a", b"", b"b\x00c", b""], None, [0, 4], SORT),
                          _request([b"a", b"b\x00c", b"", b"\x00"], None, [0, 2, 4], SORT)])
    assert answers == ["bad 1 0", "bad 1 1"]


def test_the_oracle_itself():
    """What the oracle gives on the cases whose answer can be written down by hand."""
    cases = fixture_cases()
    assert oracle(*cases["prefix"]) == ([2, 4, 1, 0, 3], [0, 2, 3, 5], [0, 3])                    # r1 r1 r1/2 r10 r10: "/" is 0x2f, "0" is 0x30
    assert oracle(*cases["one_read_scrambled"]) == ([4, 2, 0, 1, 3], [0, 1, 5], [0, 2])         # the primary, then by index
    assert oracle(*cases["two_primaries"]) == ([1, 3, 0, 4, 2], [0, 2, 5], [0, 2])
    assert oracle(*cases["same_name_adjacent_cells"]) == ([0, 1, 2, 4, 3], [0, 2, 3, 5], [0, 1, 3])
    assert oracle(*cases["empty_cells"]) == ([1, 0, 2, 4, 3], [0, 1, 3, 4, 5], [0, 0, 2, 2, 4, 4])
    assert oracle(*adjacent_cases()["recurs"], ADJACENT) == (list(range(7)), [0, 1, 2, 4, 5, 7], [0, 5])
    assert oracle([bytes([0x7f]), bytes([0x80]), bytes([0xff])][::-1], None, [0, 3]) == ([2, 1, 0], [0, 1, 2, 3], [0, 3])
