"""CPU tests of the one call from names and records in input order (oem_em_run_cells_records_names_sparse): declared with
the argument count the binding has, exported by both libraries, every argument error of the two calls it joins before
any device use, OEM_ERR_NO_DEVICE without a device, and the Python wrapper's own checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib
from oarfish_amd import build as _b
from oarfish_amd.builder import ALN_RECORD, filters_c
from tests.test_collate import ADJACENT, SORT, pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "oem_em_run_cells_records_names_sparse"
T = 40
FILTERS = dict(five_prime_clip=2 ** 32 - 1, three_prime_clip=2 ** 62, score_threshold=0.95, min_aligned_fraction=0.5,
               min_aligned_len=50, which_strand=0, score_prob_denom=5.0)


def _input():
    """Three cells (the second without records) of five records: the names of tests/test_collate.py's _input."""
    rec = np.zeros(5, dtype=ALN_RECORD)
    for i in range(5):
        rec[i] = (i % T, 10, 1500, 1400, 1000 - i, 1500, _lib.REC_HAS_SCORE, 0)
    blob, off = pack([b"r2", b"r1", b"r2", b"q", b"q"])
    return dict(F=filters_c(FILTERS), tl=np.full(T, 2000, dtype=np.uint64), rec=rec, blob=blob, off=off,
                sec=np.array([0, 0, 1, 0, 1], dtype=np.uint8), cro=np.array([0, 3, 3, 5], dtype=np.uint64))


def _call(L, F, tl, rec, blob, off, sec, cro, n_txps=T, n=5, n_cells=3, mode=SORT, bin_width=100, model=-1, out=True):
    res = C.c_void_p(1)
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    rc = getattr(L, NAME)(None if F is None else C.addressof(F), ptr(tl), n_txps, ptr(rec), n, ptr(blob), ptr(off), ptr(sec),
                          ptr(cro), n_cells, mode, bin_width, model, 2.0, 0, 100, 1e-3, None, None, None, None, None,
                          C.byref(res) if out else None)
    return rc, res, L.oem_last_error() or b""


def test_declared_exported_by_both_libraries_and_bound():
    src = open(os.path.join(ROOT, "include", "oarfish_em.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, src)
    assert m, "include/oarfish_em.h does not declare " + NAME
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 23 and args[0].startswith("const oem_filters *filters") and args[-1] == "oem_cells_result **out"
    for path in (_b.LIB_PATH, _b.TESTING_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert NAME in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, path
    assert NAME in _lib.ABI_SYMBOLS
    assert len(getattr(_lib.lib(), NAME).argtypes) == len(args)
    assert len(getattr(_lib.testing_lib(), NAME).argtypes) == len(args)
    assert _lib.lib().oem_abi_version() == 2
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert [ln for ln in doc.splitlines() if NAME in ln and ln.lstrip().startswith("|")], "INTEGRATION.md has no row for it"


def test_argument_errors_come_before_any_device_use():
    L = _lib.lib()
    a = _input()
    off_from_1 = a["off"].copy()
    off_from_1[0] = 1
    off_dec = a["off"].copy()
    off_dec[2] = 1
    cases = [   # (what is wrong, arguments, a word of the message): the records call's, then the collation's
        ("filters NULL", dict(F=None), b"bad argument"),
        ("txp_len NULL", dict(tl=None), b"bad argument"),
        ("n_txps 0", dict(n_txps=0), b"bad argument"),
        ("model 2", dict(model=2), b"model"),
        ("model -2", dict(model=-2), b"model"),
        ("bin width 0 with a model", dict(model=1, bin_width=0), b"bin width"),
        ("records NULL", dict(rec=None), b"records is NULL"),
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
        rc, res, msg = _call(L, **b)
        assert rc == _lib.OEM_ERR_ARG, (what, rc, msg)
        assert not res.value, what
        assert word in msg and NAME.encode() in msg or word == b"bin width" and word in msg, (what, msg)
    rc, _, msg = _call(L, **a, out=False)
    assert rc == _lib.OEM_ERR_ARG and b"out is NULL" in msg


def test_well_formed_input_needs_a_device():
    L = _lib.lib()
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
        with pytest.raises(oarfish_amd.OemError) as e:
            oarfish_amd.em_cells_records_sparse(FILTERS, a["tl"], a["rec"], None, a["cro"], names=(a["blob"], a["off"]),
                                                secondary=a["sec"], collate="device")
        assert e.value.code == _lib.OEM_ERR_NO_DEVICE


def test_the_wrapper_checks_its_own_arguments():
    a = _input()
    names = (a["blob"], a["off"])
    goff = np.array([0, 1, 3, 5], dtype=np.uint64)
    cgo = np.array([0, 2, 2, 3], dtype=np.uint64)
    for bad in ("gpu", "", None, "Device"):
        with pytest.raises(ValueError, match="collate"):
            oarfish_amd.em_cells_records_sparse(FILTERS, a["tl"], a["rec"], None, a["cro"], names=names, collate=bad)
    for collate in ("host", "device"):
        with pytest.raises(ValueError, match="secondary"):
            oarfish_amd.em_cells_records_sparse(FILTERS, a["tl"], a["rec"], goff, cgo, secondary=a["sec"], collate=collate)
    with pytest.raises(ValueError, match="mode"):
        oarfish_amd.em_cells_records_sparse(FILTERS, a["tl"], a["rec"], None, a["cro"], names=names, collate="device", mode="sorted")
    with pytest.raises(ValueError, match="one entry per record"):
        oarfish_amd.em_cells_records_sparse(FILTERS, a["tl"], a["rec"][:4], None, a["cro"], names=names, collate="device")
    with pytest.raises(ValueError, match="one entry per record"):
        oarfish_amd.em_cells_records_sparse(FILTERS, a["tl"], a["rec"], None, a["cro"], names=names, secondary=a["sec"][:4],
                                            collate="device")
