"""CPU tests of the sorting names session (oem_records_stream_set_sort / _push_sort / _order_copy,
``RecordsStream(names=True, mode="sort")``): declared, exported and bound; every host-visible argument and call-order
error before any device use; ``synth.cut_named_records`` with secondary flags; and the streamed host rule of
oarfish_amd/csrc/oem_collate.h (ParseBulkSortStream) held to parse_bulk_host(kCollateSort) on the concatenation, for
every single cut, every pair of cuts and one record per batch of the permuted 16-record input and for seeded random
inputs, in a stand-alone program under the address and undefined-behaviour sanitizers.
tests/test_records_stream_sort_gpu.py holds the device to the same input and cuttings."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oarfish_amd import _lib, synth
from oarfish_amd import build as _b
from oarfish_amd.builder import ALN_RECORD, RecordsStream, filters_c

from tests.records_stream_names_common import INPUT16, T, U
from tests.records_stream_sort_common import PERM16, SECONDARY16, names_list, sort_records16, sort_rule

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "parse_bulk_sort_stream_main.cpp")
EXE = os.path.join(HERE, "native", "parse_bulk_sort_stream_main")
HDR = os.path.join(ROOT, "oarfish_amd", "csrc", "oem_collate.h")
NEW = {"oem_records_stream_set_sort": 1, "oem_records_stream_push_sort": 7, "oem_records_stream_order_copy": 2}
FILTERS = dict(five_prime_clip=2 ** 32 - 1, three_prime_clip=2 ** 62, score_threshold=0.95, min_aligned_fraction=0.5,
               min_aligned_len=50, which_strand=0, score_prob_denom=5.0)
TL = np.full(T, 2000, dtype=np.uint64)


def test_declared_exported_by_both_libraries_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "oarfish_em.h")).read(), flags=re.S)
    for name, n_args in NEW.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
        assert m, "include/oarfish_em.h does not declare " + name
        assert len(m.group(1).split(",")) == n_args
        assert name in _lib.ABI_SYMBOLS
        assert len(getattr(_lib.lib(), name).argtypes) == n_args
    assert "secondary" in re.search(r"oem_records_stream_push_sort\s*\(([^;]*)\)", src).group(1)
    for path in (_b.LIB_PATH, _b.TESTING_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert set(NEW) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, path
    assert "OEM_RECORDS_STREAM_INFO_ARENA_BYTES 9u" in src and _lib.OEM_RECORDS_STREAM_INFO_ARENA_BYTES == 9
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in doc, "INTEGRATION.md does not name " + name


def _push(L, s, rec, blob, off, sec=None, n=None):
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    t = C.c_uint64(77)
    rc = L.oem_records_stream_push_sort(s, ptr(rec), len(rec) if n is None else n, ptr(blob), ptr(off), ptr(sec), C.byref(t))
    return rc, int(t.value), L.oem_last_error() or b""


def test_null_sessions_are_argument_errors():
    L = _lib.lib()
    rec, (blob, off), sec = sort_records16()
    out = np.zeros(16, dtype=np.uint64)
    assert L.oem_records_stream_set_sort(None) == _lib.OEM_ERR_ARG and b"NULL session" in L.oem_last_error()
    assert _push(L, None, rec, blob, off, sec)[0] == _lib.OEM_ERR_ARG and b"NULL session" in L.oem_last_error()
    assert L.oem_records_stream_order_copy(None, out.ctypes.data) == _lib.OEM_ERR_ARG and b"NULL session" in L.oem_last_error()


@pytest.fixture
def session():
    """a session handle, where one can be made without a device; None otherwise"""
    L = _lib.lib()
    o = _lib.RecordsStreamOptsC()
    o.n_txps, o.device, o.bin_width, o.model, o.growth_rate = T, 0, 100, -1, 2.0
    F = filters_c(FILTERS)
    h = C.c_void_p()
    rc = L.oem_records_stream_create(C.byref(o), C.addressof(F), TL.ctypes.data, C.byref(h))
    if rc == _lib.OEM_ERR_NO_DEVICE:
        yield L, None
        return
    assert rc == _lib.OEM_OK
    yield L, h
    L.oem_records_stream_destroy(h)


def test_argument_and_call_order_errors_come_before_any_device_use(session):
    L, s = session
    rec, (blob, off), sec = sort_records16()

    def moved(at, v):
        o = off.copy()
        o[at] = v
        return o

    arg_cases = [   # push_names' checks, on the calling thread before the session is looked at
        ("name_off NULL", (rec, blob, None), b"name_off is NULL"),
        ("name_off not from 0", (rec, blob, moved(0, 1)), b"name_off must start at 0"),
        ("name_off decreases", (rec, blob, moved(3, 1)), b"non-decreasing"),
        ("names NULL with bytes", (rec, None, off), b"names is NULL"),
        ("records NULL", (None, blob, off), b"records is NULL"),
    ]
    if s is None:   # no device: a session cannot exist; the create call says so, and the wrapper passes it on
        with pytest.raises(_lib.OemError) as ei:
            RecordsStream(FILTERS, TL, names=True, mode="sort")
        assert ei.value.code == _lib.OEM_ERR_NO_DEVICE
        return
    out = np.zeros(16, dtype=np.uint64)
    rc, t, msg = _push(L, s, rec, blob, off, sec)                       # before set_sort
    assert rc == _lib.OEM_ERR_STATE and t == 77 and b"not a sorting names session" in msg
    assert L.oem_records_stream_order_copy(s, out.ctypes.data) == _lib.OEM_ERR_STATE
    assert L.oem_records_stream_set_sort(s) == _lib.OEM_OK
    assert L.oem_records_stream_set_sort(s) == _lib.OEM_ERR_STATE and b"already" in L.oem_last_error()
    assert L.oem_records_stream_set_names(s, 5) == _lib.OEM_ERR_STATE
    po = _lib.ProjOptsC() if hasattr(_lib, "ProjOptsC") else None
    if po is not None:
        po.beta, po.prob_source = 10.0, 0
        assert L.oem_records_stream_set_projected(s, C.addressof(po)) == _lib.OEM_ERR_STATE
    # on a sorting session the other pushes and the plain finish are out of order
    goff = np.array([0, len(rec)], dtype=np.uint64)
    t = C.c_uint64(0)
    h = C.c_void_p(1)
    assert L.oem_records_stream_push(s, rec.ctypes.data, goff.ctypes.data, 1, C.byref(t)) == _lib.OEM_ERR_STATE
    assert b"oem_records_stream_push_sort" in L.oem_last_error()
    assert L.oem_records_stream_push_names(s, rec.ctypes.data, len(rec), blob.ctypes.data, off.ctypes.data, C.byref(t)) == _lib.OEM_ERR_STATE
    rl = np.full(1, 1500, dtype=np.uint64)
    assert L.oem_records_stream_push_projected(s, rec.ctypes.data, goff.ctypes.data, rl.ctypes.data, 1, C.byref(t)) == _lib.OEM_ERR_STATE
    assert L.oem_records_stream_finish(s, None, None, None, C.byref(h)) == _lib.OEM_ERR_STATE and not h.value
    for what, (r, b, o), word in arg_cases:
        rc, t, msg = _push(L, s, r, b, o, sec, n=len(rec))
        assert rc == _lib.OEM_ERR_ARG and t == 77 and word in msg and b"oem_records_stream_push_sort" in msg, (what, msg)
    rc, _, msg = _push(L, s, rec, blob, off, sec, n=2 ** 31 - 1)
    assert rc == _lib.OEM_ERR_ARG and b"2^31 - 2" in msg
    assert L.oem_records_stream_order_copy(s, out.ctypes.data) == _lib.OEM_ERR_STATE      # not finished yet
    assert L.oem_records_stream_names_copy(s, None, None, None, None) == _lib.OEM_ERR_STATE
    v = C.c_uint64(9)
    assert L.oem_records_stream_info(s, _lib.OEM_RECORDS_STREAM_INFO_BATCHES, C.byref(v)) == _lib.OEM_OK and v.value == 0   # no ticket was used
    assert L.oem_records_stream_info(s, _lib.OEM_RECORDS_STREAM_INFO_ARENA_BYTES, C.byref(v)) == _lib.OEM_OK and v.value == 0


def test_the_wrappers_check_their_own_arguments():
    from oarfish_amd.bulk import BulkArgs, quantify_bulk_alignments_from_record_batches
    rec, names, sec = sort_records16()
    with pytest.raises(ValueError, match="mode must be"):
        RecordsStream(FILTERS, TL, names=True, mode="sorted")
    with pytest.raises(ValueError, match="names=True"):
        RecordsStream(FILTERS, TL, mode="sort")
    with pytest.raises(ValueError, match="mode must be"):
        quantify_bulk_alignments_from_record_batches(FILTERS, ["t"] * T, [2000] * T, [], BulkArgs(output="unused"), mode="name")
    for kw in (dict(names=True, sorting=False, projected=False), dict(names=False, sorting=False, projected=False),
               dict(names=False, sorting=False, projected=True)):   # secondary= with any other mode, before the handle is touched
        s = RecordsStream.__new__(RecordsStream)
        s.__dict__.update(kw, _h=C.c_void_p())
        with pytest.raises(ValueError, match="sorting names session"):
            s.push(rec, names=names, secondary=sec)
    if _lib.device_count() == 0:
        return
    with RecordsStream(FILTERS, TL, names=True, mode="sort") as s:
        with pytest.raises(ValueError, match="one entry per record"):
            s.push(rec[:5], names=names, secondary=sec[:5])
        with pytest.raises(ValueError, match="secondary must have one entry per record"):
            s.push(rec, names=names, secondary=sec[:5])
        with pytest.raises(ValueError, match="not both"):
            s.push(rec, np.array([0, 16], dtype=np.uint64), names=names)
    with RecordsStream(FILTERS, TL, names=True) as s:                   # mode="adjacent" stays the default
        assert not s.sorting and "arena_bytes" not in s.info()


def test_cut_named_records_with_secondary_flags():
    rec, (blob, off), sec = sort_records16()
    for cuts in [(), (0,), (16,), (5, 5), (3, 11), (9, 2), tuple(range(1, 16))]:
        batches = synth.cut_named_records(rec, (blob, off), cuts, secondary=sec)
        plain = synth.cut_named_records(rec, (blob, off), cuts)
        assert len(batches) == len(plain) == len(cuts) + 1
        assert all(len(b) == 3 for b in batches) and all(len(b) == 2 for b in plain)      # a third element only when given
        assert np.array_equal(np.concatenate([b[2] for b in batches]), sec)
        for (r, nm, sc), (r2, nm2) in zip(batches, plain):
            assert np.array_equal(r, r2) and np.array_equal(nm[0], nm2[0]) and np.array_equal(nm[1], nm2[1])
            assert len(sc) == len(r) and sc.dtype == sec.dtype and sc.flags["C_CONTIGUOUS"]
    with pytest.raises(ValueError, match="secondary"):
        synth.cut_named_records(rec, (blob, off), [4], secondary=sec[:9])


def test_the_input_is_the_names_sessions_permuted_with_secondaries_before_their_primaries():
    rec, names, sec = sort_records16()
    assert sorted(PERM16) == list(range(16)) and PERM16 != sorted(PERM16)
    nl = names_list(names)
    assert nl == [INPUT16[p][1] for p in PERM16] and [int(f) for f in rec["flags"] & U] == [INPUT16[p][0] for p in PERM16]
    at = {p: k for k, p in enumerate(PERM16)}                            # where a record of INPUT16 went
    assert all(sec[at[p]] == (p in SECONDARY16) for p in range(16))
    assert at[11] < at[10] and at[9] < at[8] and at[5] < at[3]           # secondaries before their primary, and out of order
    order, group_off = sort_rule(rec, names, sec)
    assert [nl[i] for i in order[group_off[:-1].astype(np.int64)]] == [b"ACGTACGTAC", b"r1", b"r3", b"r5", b"read2"]
    assert list(np.diff(group_off)) == [2, 1, 1, 4, 3]
    assert [int(i) for i in order[:2]] == [at[8], at[9]] and int(order[4]) == at[10] and int(order[8]) == at[2]   # the primaries lead


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-o", EXE, SRC])
    return EXE


def test_streamed_sort_rule_equals_the_whole_parse_for_every_cutting_under_sanitizers(exe):
    rec, names, sec = sort_records16()
    nl = names_list(names)
    text = f"{len(nl)}\n" + "".join(f"{int(rec['flags'][i] & U)} {int(sec[i])} {nl[i].hex() or '-'}\n" for i in range(len(nl)))
    r = subprocess.run([exe, "20261020", "400"], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    order, group_off = sort_rule(rec, names, sec)
    want = f"ok {2 * (17 + 136 + 1)} {len(group_off) - 1} 5 400 | " + " ".join(map(str, order)) + " | " + " ".join(map(str, group_off))
    assert r.stdout.strip() == want
