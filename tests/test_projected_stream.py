"""CPU tests of the projected session (oem_records_stream_set_projected / _push_projected): declared, exported and bound;
every host-visible argument and call-order error before any device use; the wrapper's own checks; and
``synth.cut_projected_records``.  tests/test_projected_stream_gpu.py holds the device to the one call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oarfish_amd import _lib, synth
from oarfish_amd import build as _b
from oarfish_amd.builder import PROJ_RECORD, RecordsStream, filters_c, proj_opts_c

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ["oem_records_stream_set_projected", "oem_records_stream_push_projected"]
T = 7
FILTERS = dict(five_prime_clip=2 ** 32 - 1, three_prime_clip=2 ** 62, score_threshold=0.95, min_aligned_fraction=0.5,
               min_aligned_len=50, which_strand=0, score_prob_denom=5.0)


def batch3():
    """three groups of 2, 0 and 1 records"""
    rec = np.zeros(3, dtype=PROJ_RECORD)
    rec["similarity"], rec["end"], rec["aligned_len"], rec["query_aligned_len"] = 0.9, 1500, 1400, 1400
    rec["ref_id"] = [0, 1, 2]
    return rec, np.array([0, 2, 2, 3], dtype=np.uint64), np.array([1500, 1500, 1500], dtype=np.uint64)


def test_declared_exported_by_both_libraries_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "oarfish_em.h")).read(), flags=re.S)
    n_args = {NEW[0]: 2, NEW[1]: 6}
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
        assert m, "include/oarfish_em.h does not declare " + name
        assert len(m.group(1).split(",")) == n_args[name]
        assert name in _lib.ABI_SYMBOLS
        assert len(getattr(_lib.lib(), name).argtypes) == n_args[name]
    for path in (_b.LIB_PATH, _b.TESTING_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert set(NEW) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, path
    full = open(os.path.join(ROOT, "include", "oarfish_em.h")).read()
    assert "OEM_RECORDS_STREAM_INFO_HOST_FINISHED 8u" in full and _lib.OEM_RECORDS_STREAM_INFO_HOST_FINISHED == 8
    assert C.sizeof(_lib.RecordsStreamOptsC) == 48
    assert _lib.lib().oem_abi_version() == 2
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in doc, "INTEGRATION.md does not name " + name


def _push(L, s, rec, off, rl, n=None):
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    t = C.c_uint64(77)
    rc = L.oem_records_stream_push_projected(s, ptr(rec), ptr(off), ptr(rl), len(rl) if n is None else n, C.byref(t))
    return rc, int(t.value), L.oem_last_error() or b""


def test_null_sessions_are_argument_errors():
    L = _lib.lib()
    po = proj_opts_c()
    assert L.oem_records_stream_set_projected(None, C.addressof(po)) == _lib.OEM_ERR_ARG and b"NULL session" in L.oem_last_error()
    rc, t, msg = _push(L, None, *batch3())
    assert rc == _lib.OEM_ERR_ARG and t == 77 and b"NULL session" in msg


def _session(L):
    o = _lib.RecordsStreamOptsC()
    o.n_txps, o.device, o.bin_width, o.model, o.growth_rate = T, 0, 100, -1, 2.0
    F = filters_c(FILTERS)
    tl = np.full(T, 2000, dtype=np.uint64)
    h = C.c_void_p()
    rc = L.oem_records_stream_create(C.byref(o), C.addressof(F), tl.ctypes.data, C.byref(h))
    return rc, h


@pytest.fixture
def sessions():
    """three session handles, where one can be made without a device; None otherwise"""
    L = _lib.lib()
    made = []
    for _ in range(3):
        rc, h = _session(L)
        if rc == _lib.OEM_ERR_NO_DEVICE:
            yield L, None
            return
        assert rc == _lib.OEM_OK
        made.append(h)
    yield L, made
    for h in made:
        L.oem_records_stream_destroy(h)


def _batches(L, s):
    v = C.c_uint64(9)
    assert L.oem_records_stream_info(s, _lib.OEM_RECORDS_STREAM_INFO_BATCHES, C.byref(v)) == _lib.OEM_OK
    return int(v.value)


def test_argument_and_call_order_errors_come_before_any_device_use(sessions):
    L, made = sessions
    rec, off, rl = batch3()
    if made is None:   # no device: a session cannot exist; the create call says so, and the wrapper passes it on
        with pytest.raises(_lib.OemError) as ei:
            RecordsStream(FILTERS, np.full(T, 2000, dtype=np.uint64), projected=True)
        assert ei.value.code == _lib.OEM_ERR_NO_DEVICE
        return
    s, named, plain = made
    po = proj_opts_c(10.0, "combined")
    h = C.c_void_p(1)

    # a plain session: the projected push is out of order; set_projected checks its options first
    rc, t, msg = _push(L, s, rec, off, rl)
    assert rc == _lib.OEM_ERR_STATE and t == 77 and b"not a projected session" in msg
    assert L.oem_records_stream_set_projected(s, None) == _lib.OEM_ERR_ARG and b"popts is NULL" in L.oem_last_error()
    for bad in (-1, 3):
        bo = _lib.ProjOptsC(10.0, bad)
        assert L.oem_records_stream_set_projected(s, C.addressof(bo)) == _lib.OEM_ERR_ARG
        assert b"prob_source %d (0 similarity, 1 score or 2 combined)" % bad in L.oem_last_error()
    assert L.oem_records_stream_set_projected(s, C.addressof(po)) == _lib.OEM_OK
    assert L.oem_records_stream_set_projected(s, C.addressof(po)) == _lib.OEM_ERR_STATE and b"already" in L.oem_last_error()

    # a projected session: the plain and the names calls are out of order
    assert L.oem_records_stream_set_names(s, 5) == _lib.OEM_ERR_STATE and b"projected session" in L.oem_last_error()
    arec = np.zeros(3, dtype=np.dtype([("b", "u1", 40)]))
    t = C.c_uint64(77)
    assert L.oem_records_stream_push(s, arec.ctypes.data, off.ctypes.data, 3, C.byref(t)) == _lib.OEM_ERR_STATE and t.value == 77
    assert b"oem_records_stream_push_projected" in L.oem_last_error()
    blob, noff = np.frombuffer(b"abc", dtype=np.uint8), np.array([0, 1, 2, 3], dtype=np.uint64)
    assert L.oem_records_stream_push_names(s, arec.ctypes.data, 3, blob.ctypes.data, noff.ctypes.data, C.byref(t)) == _lib.OEM_ERR_STATE
    assert t.value == 77
    assert L.oem_records_stream_finish_names(s, None, None, None, C.byref(h)) == _lib.OEM_ERR_STATE and not h.value
    assert L.oem_records_stream_names_copy(s, None, None, None, None) == _lib.OEM_ERR_STATE

    # a names session: neither set_projected nor the projected push
    assert L.oem_records_stream_set_names(named, 5) == _lib.OEM_OK
    assert L.oem_records_stream_set_projected(named, C.addressof(po)) == _lib.OEM_ERR_STATE and b"names session" in L.oem_last_error()
    rc, t, msg = _push(L, named, rec, off, rl)
    assert rc == _lib.OEM_ERR_STATE and t == 77 and b"not a projected session" in msg

    # the argument errors of a push: the batch is rejected, the ticket untouched, no ticket used
    def moved(at, v):
        o = off.copy()
        o[at] = v
        return o

    arg_cases = [
        ("group_off NULL", (rec, None, rl), b"group_off is NULL"),
        ("group_off not from 0", (rec, moved(0, 1), rl), b"group_off[0] must be 0"),
        ("group_off decreases", (rec, moved(2, 1), rl), b"decreases at group 1"),
        ("read_len NULL", (rec, off, None), b"read_len is NULL"),
        ("records NULL with records present", (None, off, rl), b"records is NULL"),
    ]
    for what, (r, o, l), word in arg_cases:
        rc, t, msg = _push(L, s, r, o, l, n=3)
        assert rc == _lib.OEM_ERR_ARG and t == 77 and word in msg and b"oem_records_stream_push_projected" in msg, (what, msg)
    rc, t, msg = _push(L, s, rec, off, rl, n=2 ** 31 - 1)
    assert rc == _lib.OEM_ERR_ARG and t == 77 and b"2^31 - 2" in msg
    assert _batches(L, s) == 0

    # after a push, and after finish: set_projected is out of order
    goff = np.array([0, 3], dtype=np.uint64)
    assert L.oem_records_stream_push(plain, arec.ctypes.data, goff.ctypes.data, 1, None) == _lib.OEM_OK
    assert L.oem_records_stream_set_projected(plain, C.addressof(po)) == _lib.OEM_ERR_STATE and b"pushed already" in L.oem_last_error()
    v = C.c_uint64(9)
    assert L.oem_records_stream_info(plain, _lib.OEM_RECORDS_STREAM_INFO_HOST_FINISHED, C.byref(v)) == _lib.OEM_OK and v.value == 0
    rc, h2 = _session(L)
    assert rc == _lib.OEM_OK
    try:
        st = C.c_void_p()
        assert L.oem_records_stream_finish(h2, None, None, None, C.byref(st)) == _lib.OEM_OK
        L.oem_store_destroy(st)
        assert L.oem_records_stream_set_projected(h2, C.addressof(po)) == _lib.OEM_ERR_STATE and b"finished" in L.oem_last_error()
    finally:
        L.oem_records_stream_destroy(h2)


def test_the_wrapper_checks_its_own_arguments():
    rec, off, rl = batch3()
    tl = np.full(T, 2000, dtype=np.uint64)
    with pytest.raises(ValueError, match="not both"):      # before any session is made
        RecordsStream(FILTERS, tl, names=True, projected=True)
    with pytest.raises(ValueError, match="prob_source"):
        RecordsStream(FILTERS, tl, projected=True, prob_source="best")
    if _lib.device_count() == 0:
        return
    with RecordsStream(FILTERS, tl) as s:
        with pytest.raises(ValueError, match="projected session"):
            s.push(rec, off, read_len=rl)
    with RecordsStream(FILTERS, tl, names=True) as s:
        with pytest.raises(ValueError, match="projected session"):
            s.push(rec, names=["a", "b", "c"], read_len=rl)
    with RecordsStream(FILTERS, tl, projected=True) as s:
        with pytest.raises(ValueError, match="read_len"):
            s.push(rec, off)
        with pytest.raises(ValueError, match="read_len"):
            s.push(rec, read_len=rl)
        with pytest.raises(ValueError, match="names"):
            s.push(rec, off, names=["a", "b", "c"], read_len=rl)
        with pytest.raises(ValueError, match="n_groups entries"):
            s.push(rec, off, read_len=rl[:2])
        assert "host_finished" in s.info() and "row_name_bytes" not in s.info()
    with RecordsStream(FILTERS, tl) as s:
        assert "host_finished" not in s.info()


def test_cut_projected_records():
    spr = synth.make_projected_records(synth.make_store(200, 40, kbar=3, seed=5))
    G = len(spr.group_off) - 1
    assert G > 200
    for sizes in ([], [G], [0], [1, 0, 63, 64, 65], [0, 0, G, 0], [G - 1], [50] * 4):
        batches = synth.cut_projected_records(spr, sizes)
        want = list(sizes) + ([G - sum(sizes)] if sum(sizes) < G or not sizes else [])
        assert [len(b[2]) for b in batches] == want
        for r, o, l in batches:
            assert r.dtype == PROJ_RECORD and o.dtype == np.uint64 and l.dtype == np.uint64
            assert o[0] == 0 and len(o) == len(l) + 1 and int(o[-1]) == len(r)
        assert np.array_equal(np.concatenate([b[0] for b in batches]), spr.records)
        assert np.array_equal(np.concatenate([b[2] for b in batches]), spr.read_len)
        off, base = [np.zeros(1, dtype=np.uint64)], 0
        for r, o, _ in batches:
            off.append(o[1:] + np.uint64(base))
            base += len(r)
        assert np.array_equal(np.concatenate(off), spr.group_off)
    empty = synth.cut_projected_records(spr, [0])[0]
    assert len(empty[0]) == 0 and list(empty[1]) == [0] and len(empty[2]) == 0
    triple = synth.cut_projected_records((spr.records, spr.group_off, spr.read_len), [10])
    again = synth.cut_projected_records(spr, [10])
    assert all(np.array_equal(x, y) for a, b in zip(triple, again) for x, y in zip(a, b))
    for bad in ([G + 1], [-1]):
        with pytest.raises(ValueError):
            synth.cut_projected_records(spr, bad)
