"""CPU tests of the names session (oem_records_stream_set_names / _push_names / _finish_names / _names_copy): declared,
exported and bound; every host-visible argument and call-order error before any device use; ``synth.cut_named_records``;
and the streamed host rule of oarfish_amd/csrc/oem_collate.h (ParseBulkStream) held to parse_bulk_host on the
concatenation, for every single cut, every pair of cuts and one record per batch of a 16-record input, in a stand-alone
program under the address and undefined-behaviour sanitizers.  tests/test_records_stream_names_gpu.py holds the device
to the same input and cuttings."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oarfish_amd import _lib, synth
from oarfish_amd import build as _b
from oarfish_amd.builder import ALN_RECORD, RecordsStream, filters_c

from tests.records_stream_names_common import HEADS16, INPUT16, SIZES16, T, U, cuttings16, records16

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "parse_bulk_stream_main.cpp")
EXE = os.path.join(HERE, "native", "parse_bulk_stream_main")
HDR = os.path.join(ROOT, "oarfish_amd", "csrc", "oem_collate.h")
NEW = ["oem_records_stream_set_names", "oem_records_stream_push_names", "oem_records_stream_finish_names",
       "oem_records_stream_names_copy"]
FILTERS = dict(five_prime_clip=2 ** 32 - 1, three_prime_clip=2 ** 62, score_threshold=0.95, min_aligned_fraction=0.5,
               min_aligned_len=50, which_strand=0, score_prob_denom=5.0)


def test_declared_exported_by_both_libraries_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "oarfish_em.h")).read(), flags=re.S)
    n_args = {NEW[0]: 2, NEW[1]: 6, NEW[2]: 5, NEW[3]: 5}
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
        assert m, "include/oarfish_em.h does not declare " + name
        assert len(m.group(1).split(",")) == n_args[name]
        assert name in _lib.ABI_SYMBOLS
        assert len(getattr(_lib.lib(), name).argtypes) == n_args[name]
    assert "secondary" not in re.search(r"oem_records_stream_push_names\s*\(([^;]*)\)", src).group(1)
    for path in (_b.LIB_PATH, _b.TESTING_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert set(NEW) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, path
    assert "OEM_RECORDS_STREAM_INFO_ROW_NAME_BYTES 7u" in src and _lib.OEM_RECORDS_STREAM_INFO_ROW_NAME_BYTES == 7
    assert C.sizeof(_lib.RecordsStreamOptsC) == 48
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in doc, "INTEGRATION.md does not name " + name


def _push(L, s, rec, blob, off, n=None):
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    t = C.c_uint64(77)
    rc = L.oem_records_stream_push_names(s, ptr(rec), len(rec) if n is None else n, ptr(blob), ptr(off), C.byref(t))
    return rc, int(t.value), L.oem_last_error() or b""


def test_null_sessions_are_argument_errors():
    L = _lib.lib()
    rec, (blob, off) = records16()
    h = C.c_void_p(1)
    assert L.oem_records_stream_set_names(None, 10) == _lib.OEM_ERR_ARG and b"NULL session" in L.oem_last_error()
    assert _push(L, None, rec, blob, off)[0] == _lib.OEM_ERR_ARG and b"NULL session" in L.oem_last_error()
    assert L.oem_records_stream_finish_names(None, None, None, None, C.byref(h)) == _lib.OEM_ERR_ARG and not h.value
    assert b"NULL session" in L.oem_last_error()
    assert L.oem_records_stream_finish_names(None, None, None, None, None) == _lib.OEM_ERR_ARG
    assert L.oem_records_stream_names_copy(None, None, None, None, None) == _lib.OEM_ERR_ARG and b"NULL session" in L.oem_last_error()


@pytest.fixture
def session():
    """a session handle, where one can be made without a device; None otherwise"""
    L = _lib.lib()
    o = _lib.RecordsStreamOptsC()
    o.n_txps, o.device, o.bin_width, o.model, o.growth_rate = T, 0, 100, -1, 2.0
    F = filters_c(FILTERS)
    tl = np.full(T, 2000, dtype=np.uint64)
    h = C.c_void_p()
    rc = L.oem_records_stream_create(C.byref(o), C.addressof(F), tl.ctypes.data, C.byref(h))
    if rc == _lib.OEM_ERR_NO_DEVICE:
        yield L, None
        return
    assert rc == _lib.OEM_OK
    yield L, h
    L.oem_records_stream_destroy(h)


def test_argument_and_call_order_errors_come_before_any_device_use(session):
    L, s = session
    rec, (blob, off) = records16()

    def moved(at, v):
        o = off.copy()
        o[at] = v
        return o

    arg_cases = [   # checked on the calling thread before the session is looked at: a NULL session never hides them
        ("name_off NULL", (rec, blob, None), b"name_off is NULL"),
        ("name_off not from 0", (rec, blob, moved(0, 1)), b"name_off must start at 0"),
        ("name_off decreases", (rec, blob, moved(3, 1)), b"non-decreasing"),
        ("names NULL with bytes", (rec, None, off), b"names is NULL"),
        ("records NULL", (None, blob, off), b"records is NULL"),
    ]
    if s is None:   # no device: a session cannot exist; the create call says so, and the wrapper passes it on
        with pytest.raises(_lib.OemError) as ei:
            RecordsStream(FILTERS, np.full(T, 2000, dtype=np.uint64), names=True)
        assert ei.value.code == _lib.OEM_ERR_NO_DEVICE
        return
    # before set_names: the names calls are out of order, the plain ones are not
    h = C.c_void_p(1)
    rc, t, msg = _push(L, s, rec, blob, off)
    assert rc == _lib.OEM_ERR_STATE and t == 77 and b"not a names session" in msg
    assert L.oem_records_stream_finish_names(s, None, None, None, C.byref(h)) == _lib.OEM_ERR_STATE and not h.value
    assert L.oem_records_stream_names_copy(s, None, None, None, None) == _lib.OEM_ERR_STATE
    assert L.oem_records_stream_set_names(s, 5) == _lib.OEM_OK
    assert L.oem_records_stream_set_names(s, 5) == _lib.OEM_ERR_STATE and b"already" in L.oem_last_error()
    # after set_names: the plain calls are out of order
    goff = np.array([0, len(rec)], dtype=np.uint64)
    t = C.c_uint64(0)
    assert L.oem_records_stream_push(s, rec.ctypes.data, goff.ctypes.data, 1, C.byref(t)) == _lib.OEM_ERR_STATE
    assert L.oem_records_stream_finish(s, None, None, None, C.byref(h)) == _lib.OEM_ERR_STATE and not h.value
    for what, (r, b, o), word in arg_cases:
        rc, t, msg = _push(L, s, r, b, o, n=len(rec))
        assert rc == _lib.OEM_ERR_ARG and t == 77 and word in msg and b"oem_records_stream_push_names" in msg, (what, msg)
    rc, _, msg = _push(L, s, rec, blob, off, n=2 ** 31 - 1)
    assert rc == _lib.OEM_ERR_ARG and b"2^31 - 2" in msg
    assert L.oem_records_stream_names_copy(s, None, None, blob.ctypes.data, None) == _lib.OEM_ERR_ARG
    assert L.oem_records_stream_names_copy(s, None, None, None, None) == _lib.OEM_ERR_STATE       # not finished yet
    v = C.c_uint64(9)
    assert L.oem_records_stream_info(s, _lib.OEM_RECORDS_STREAM_INFO_BATCHES, C.byref(v)) == _lib.OEM_OK and v.value == 0   # no ticket was used


def test_the_wrapper_checks_its_own_arguments():
    rec, names = records16()
    batches = synth.cut_named_records(rec, names, [3])
    assert len(batches) == 2
    if _lib.device_count() == 0:
        return
    with RecordsStream(FILTERS, np.full(T, 2000, dtype=np.uint64), names=True) as s:
        with pytest.raises(ValueError, match="one entry per record"):
            s.push(rec[:5], names=names)
        with pytest.raises(ValueError, match="not both"):
            s.push(rec, np.array([0, 16], dtype=np.uint64), names=names)
        with pytest.raises(ValueError, match="group_off"):
            s.push(rec)


def test_cut_named_records():
    rec, (blob, off) = records16()
    names = [nm for _, nm in INPUT16]
    for cuts in cuttings16() + [(5, 5), (0, 0, 16, 16), (9, 2)]:
        batches = synth.cut_named_records(rec, (blob, off), cuts)
        assert len(batches) == len(cuts) + 1
        assert np.array_equal(np.concatenate([b[0] for b in batches]), rec)
        got = []
        for r, (bl, o) in batches:
            assert r.dtype == ALN_RECORD and o.dtype == np.uint64 and o[0] == 0 and len(o) == len(r) + 1 and int(o[-1]) == len(bl)
            got += [bytes(bl[int(o[i]):int(o[i + 1])]) for i in range(len(r))]
        assert got == names
        edges = [0] + sorted(cuts) + [16]
        assert [len(b[0]) for b in batches] == [b - a for a, b in zip(edges[:-1], edges[1:])]
    with pytest.raises(ValueError):
        synth.cut_named_records(rec, (blob, off), [17])
    again = synth.cut_named_records(rec, (blob, off), [4, 9])
    assert all(np.array_equal(a[1][0], b[1][0]) for a, b in zip(again, synth.cut_named_records(rec, (blob, off), [4, 9])))


def test_the_input_is_what_the_issue_asks_for():
    flags = [f for f, _ in INPUT16]
    names = [nm for _, nm in INPUT16]
    assert len(INPUT16) == 16 and flags[0] == U and flags[-1] == U
    mapped = [i for i in range(16) if not flags[i]]
    runs, prev = [], None
    for i in mapped:
        if names[i] != prev:
            runs.append([])
        runs[-1].append(i)
        prev = names[i]
    assert [len(r) for r in runs] == SIZES16 == [1, 3, 1, 2, 4] and [r[0] for r in runs] == HEADS16
    assert flags[6] == U and names[6] == b"" and names[5] != names[7]            # between two reads, with an empty name
    assert flags[4] == U and names[3] == names[4] == names[5]                    # inside a read, with the read's name
    assert flags[12] == U and names[11] == names[13] != names[12]                # inside a read, under another name
    cs = cuttings16()
    assert len(cs) == 17 + 136 + 1 and len(set(cs)) == len(cs)


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-o", EXE, SRC])
    return EXE


def test_streamed_host_rule_equals_the_whole_parse_for_every_cutting_under_sanitizers(exe):
    text = f"{len(INPUT16)}\n" + "".join(f"{f} {nm.hex() or '-'}\n" for f, nm in INPUT16)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    want = "ok 154 5 5 | " + " ".join(map(str, SIZES16)) + " | " + " ".join(map(str, HEADS16))
    assert r.stdout.strip() == want
