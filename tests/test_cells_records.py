"""CPU tests of the records form of the per-cell calls (oem_em_run_cells_records_sparse, oem_cells_result_discard_tables,
oem_cells_stream_set_filters, oem_cells_stream_push_records): declared, exported by both libraries, bound, and every
argument error comes before any device use -- on a box without a device a well-formed call is OEM_ERR_NO_DEVICE."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from oarfish_amd import _lib, synth
from oarfish_amd import build as _b
from oarfish_amd.builder import ALN_RECORD, filters_c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["oem_em_run_cells_records_sparse", "oem_cells_result_discard_tables", "oem_cells_stream_set_filters",
                "oem_cells_stream_push_records"]
T = 40


def _input():
    """Three cells (the second without groups) of four reads."""
    F = filters_c(dict(five_prime_clip=2 ** 32 - 1, three_prime_clip=2 ** 62, score_threshold=0.95, min_aligned_fraction=0.5,
                       min_aligned_len=50, which_strand=0, score_prob_denom=5.0))
    tl = np.full(T, 2000, dtype=np.uint64)
    rec = np.zeros(6, dtype=ALN_RECORD)
    for i in range(6):
        rec[i] = (i % T, 10, 1500, 1400, 1000 - i, 1500, _lib.REC_HAS_SCORE, 0)
    goff = np.array([0, 2, 3, 5, 6], dtype=np.uint64)
    cgo = np.array([0, 2, 2, 4], dtype=np.uint64)
    return F, tl, rec, goff, cgo


def _call(L, F, tl, rec, goff, cgo, n_txps=T, n_groups=None, n_cells=None, bin_width=100, model=-1, out=True):
    res = C.c_void_p(1)
    rc = L.oem_em_run_cells_records_sparse(
        None if F is None else C.addressof(F), None if tl is None else tl.ctypes.data, n_txps,
        None if rec is None else rec.ctypes.data, None if goff is None else goff.ctypes.data,
        len(goff) - 1 if n_groups is None else n_groups, None if cgo is None else cgo.ctypes.data,
        len(cgo) - 1 if n_cells is None else n_cells, bin_width, model, 2.0, 0, 100, 1e-3, None,
        C.byref(res) if out else None)
    return rc, res, L.oem_last_error() or b""


def test_declared_exported_by_both_libraries_and_bound():
    src = open(os.path.join(ROOT, "include", "oarfish_em.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(oem_[a-z0-9_]+)\s*\(", src))
    L = _lib.lib()
    for path in (_b.LIB_PATH, _b.TESTING_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        for name in ENTRY_POINTS:
            assert name in exported, (path, name)
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert name in _lib.ABI_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    assert L.oem_abi_version() == 2


def test_argument_errors_come_before_any_device_use():
    L = _lib.lib()
    F, tl, rec, goff, cgo = _input()
    bad_first = goff.copy()
    bad_first[0] = 1
    dec = goff.copy()
    dec[2] = 1
    cases = [   # (what is wrong, arguments, a word of the message)
        ("filters NULL", dict(F=None), b"bad argument"),
        ("txp_len NULL", dict(tl=None), b"bad argument"),
        ("n_txps 0", dict(n_txps=0), b"bad argument"),
        ("model 2", dict(model=2), b"model"),
        ("model -2", dict(model=-2), b"model"),
        ("bin width 0 with a model", dict(model=1, bin_width=0), b"bin width"),
        ("group_off NULL", dict(goff=None, n_groups=4), b"group_off is NULL"),
        ("group_off not from 0", dict(goff=bad_first), b"group_off[0]"),
        ("group_off decreases", dict(goff=dec), b"group_off decreases at group 1"),
        ("records NULL", dict(rec=None), b"records is NULL"),
        ("cell_group_off NULL", dict(cgo=None, n_cells=3), b"cell_group_off is NULL"),
        ("cell_group_off not from 0", dict(cgo=np.array([1, 2, 2, 4], dtype=np.uint64)), b"cell_group_off[0]"),
        ("cell_group_off decreases", dict(cgo=np.array([0, 3, 2, 4], dtype=np.uint64)), b"cell_group_off decreases at cell 1"),
        ("cell_group_off short of n_groups", dict(cgo=np.array([0, 2, 2, 3], dtype=np.uint64)), b"n_groups"),
        ("cell_group_off past n_groups", dict(cgo=np.array([0, 2, 2, 5], dtype=np.uint64)), b"n_groups"),
    ]
    for what, kw, word in cases:
        a = dict(F=F, tl=tl, rec=rec, goff=goff, cgo=cgo)
        a.update(kw)
        rc, res, msg = _call(L, **a)
        assert rc == _lib.OEM_ERR_ARG, (what, rc, msg)
        assert not res.value, what
        assert word in msg and b"oem_em_run_cells_records_sparse" in msg or word == b"bin width" and word in msg, (what, msg)
    rc, _, msg = _call(L, F, tl, rec, goff, cgo, out=False)
    assert rc == _lib.OEM_ERR_ARG and b"out is NULL" in msg


def test_well_formed_input_needs_a_device():
    L = _lib.lib()
    for model in (-1, 0, 1):
        rc, res, msg = _call(L, *_input(), model=model)
        if _lib.device_count() > 0:
            assert rc == _lib.OEM_OK and res.value, msg
            L.oem_cells_result_destroy(res)
        else:
            assert rc == _lib.OEM_ERR_NO_DEVICE and not res.value, (rc, msg)
    if _lib.device_count() == 0:
        import oarfish_amd
        F, tl, rec, goff, cgo = _input()
        try:
            oarfish_amd.em_cells_records_sparse(F, tl, rec, goff, cgo)
        except oarfish_amd.OemError as e:
            assert e.code == _lib.OEM_ERR_NO_DEVICE
        else:
            raise AssertionError("em_cells_records_sparse without a device must raise")


def test_null_handles():
    L = _lib.lib()
    dt = _lib.DiscardTableC()
    assert L.oem_cells_result_discard_tables(None, C.addressof(dt)) == _lib.OEM_ERR_ARG
    assert b"oem_cells_result_discard_tables" in L.oem_last_error()
    F, tl, rec, goff, _ = _input()
    assert L.oem_cells_stream_set_filters(None, C.addressof(F), tl.ctypes.data) == _lib.OEM_ERR_ARG
    t = C.c_uint64(0)
    assert L.oem_cells_stream_push_records(None, rec.ctypes.data, goff.ctypes.data, 4, C.byref(t)) == _lib.OEM_ERR_ARG


def test_make_cell_records_is_make_records_per_cell():
    """synth.make_cell_records: the cells' records one after the other over one annotation, with what the filter must
    report per cell; the Python restatement of the filter agrees on a cell."""
    from oracle import filter_py as fp
    cells = synth.make_cells(3, 60, T, kbar=3.0, seed=11)
    cr = synth.make_cell_records(cells, T, seed=5)
    assert len(cr.cell_group_off) == 4 and int(cr.cell_group_off[-1]) == len(cr.group_off) - 1 == len(cr.kept)
    assert int(cr.group_off[-1]) == len(cr.records) and len(cr.discard) == 3 and len(cr.txp_len) == T
    again = synth.make_cell_records(cells, T, seed=5)
    assert again.records.tobytes() == cr.records.tobytes() and np.array_equal(again.group_off, cr.group_off)
    F = fp.Filters(**cr.filters)
    c = 1
    g0, g1 = int(cr.cell_group_off[c]), int(cr.cell_group_off[c + 1])
    ref = fp.Store()
    for g in range(g0, g1):
        grp = []
        for x in cr.records[int(cr.group_off[g]):int(cr.group_off[g + 1])]:
            fl = int(x["flags"])
            grp.append(fp.Rec(int(x["ref_id"]), int(x["aln_start"]), int(x["aln_end"]), int(x["aln_span"]),
                              int(x["score"]) if fl & _lib.REC_HAS_SCORE else None,
                              int(x["seq_len"]) if int(x["seq_len"]) >= 0 else None, unmapped=bool(fl & _lib.REC_UNMAPPED),
                              reverse=bool(fl & _lib.REC_REVERSE), supp=bool(fl & _lib.REC_SUPPLEMENTARY)))
        assert fp.add_group(ref, F, [int(v) for v in cr.txp_len], grp) == int(cr.kept[g])
    r0, r1 = int(cells[0][c]), int(cells[0][c + 1])
    assert ref.tid == [int(t) for t in cells[2][int(cells[1][r0]):int(cells[1][r1])]]
    empty = synth.make_cell_records((np.zeros(2, np.uint64), np.zeros(1, np.uint64), np.zeros(0, np.uint32),
                                     np.zeros(0, np.float32)), T, seed=5)
    assert list(empty.cell_group_off) == [0, 0] and len(empty.records) == 0 and empty.filters == cr.filters
