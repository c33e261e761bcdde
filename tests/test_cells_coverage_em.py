"""CPU tests of the fused per-cell coverage model + EM (oem_em_run_cells_coverage_sparse / em_cells_coverage_sparse):
the entry point is exported and declared, every invalid argument is refused with OEM_ERR_ARG before any device use,
a valid call without a device fails with OEM_ERR_NO_DEVICE, and the Python wrapper checks its own arguments."""
import ctypes as C
import os

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "oarfish_em.h")


def _cells():
    """Two cells of two reads each over three transcripts, with probabilities and coordinates."""
    cell_off = np.array([0, 2, 4], dtype=np.uint64)
    rp = np.array([0, 1, 3, 4, 6], dtype=np.uint64)
    tid = np.array([0, 1, 2, 2, 0, 1], dtype=np.uint32)
    p = np.array([1.0, 0.5, 0.5, 1.0, 0.3, 0.7], dtype=np.float32)
    start = np.array([0, 10, 100, 50, 200, 0], dtype=np.uint32)
    end = np.array([300, 400, 500, 700, 600, 250], dtype=np.uint32)
    txp_len = np.array([800, 900, 1000], dtype=np.uint64)
    return cell_off, rp, tid, p, start, end, txp_len


def _call(cell_off, rp, tid, p, start, end, txp_len, n_txps=3, bin_width=100, model=1, nnz=None, n_reads=None,
          null=None, out=True):
    nnz = len(tid) if nnz is None else nnz
    n_reads = len(rp) - 1 if n_reads is None else n_reads
    arrs = dict(cell_row_off=cell_off, row_ptr=rp, tid=tid, p=p, start=start, end=end, txp_len=txp_len)
    ptr = {k: (None if k == null else v.ctypes.data) for k, v in arrs.items()}
    res = C.c_void_p()
    rc = _lib.lib().oem_em_run_cells_coverage_sparse(
        ptr["cell_row_off"], len(cell_off) - 1, ptr["row_ptr"], ptr["tid"], ptr["p"], ptr["start"], ptr["end"],
        ptr["txp_len"], n_reads, nnz, n_txps, bin_width, model, 2.0, 0, 100, 1e-3, None,
        C.byref(res) if out else None)
    if res.value:
        _lib.lib().oem_cells_result_destroy(res)
    if rc != _lib.OEM_OK and out:
        assert not res.value, "a failed call returned a result"
    return rc


def _err():
    return _lib.lib().oem_last_error()


def test_entry_point_is_exported_and_declared():
    name = "oem_em_run_cells_coverage_sparse"
    assert name in _lib.ABI_SYMBOLS
    assert hasattr(_lib.lib(), name)
    with open(HEADER) as f:
        assert f"int {name}(" in f.read()
    assert callable(oarfish_amd.em_cells_coverage_sparse) and "em_cells_coverage_sparse" in oarfish_amd.__all__


@pytest.mark.parametrize("which", ["cell_row_off", "row_ptr", "tid", "p", "start", "end", "txp_len"])
def test_null_pointers_are_refused(which):
    assert _call(*_cells(), null=which) == _lib.OEM_ERR_ARG
    assert b"NULL" in _err()


def test_null_result_handle_is_refused():
    assert _call(*_cells(), out=False) == _lib.OEM_ERR_ARG


def test_bin_width_model_and_n_txps():
    args = _cells()
    assert _call(*args, bin_width=0) == _lib.OEM_ERR_ARG
    assert b"bin width" in _err()
    for m in (-1, 2):
        assert _call(*args, model=m) == _lib.OEM_ERR_ARG
        assert b"model" in _err()
    assert _call(*args, n_txps=0) == _lib.OEM_ERR_ARG
    assert _call(*args, n_txps=(1 << 31) - 1) == _lib.OEM_ERR_ARG
    assert b"2^31" in _err()


def test_counts_of_2_to_the_32_are_refused_without_wrapping():
    assert _call(*_cells(), nnz=1 << 32) == _lib.OEM_ERR_ARG
    assert b"2^32" in _err()
    assert _call(*_cells(), n_reads=1 << 32) == _lib.OEM_ERR_ARG
    assert b"2^32" in _err()


def test_cell_row_off_must_span_all_reads_and_not_decrease():
    cell_off, rp, tid, p, s, e, tl = _cells()
    assert _call(np.array([1, 2, 4], dtype=np.uint64), rp, tid, p, s, e, tl) == _lib.OEM_ERR_ARG
    assert b"cell_row_off" in _err()
    assert _call(np.array([0, 2, 3], dtype=np.uint64), rp, tid, p, s, e, tl) == _lib.OEM_ERR_ARG
    assert b"cell_row_off" in _err()
    assert _call(np.array([0, 3, 2, 4], dtype=np.uint64), rp, tid, p, s, e, tl) == _lib.OEM_ERR_ARG
    assert b"non-decreasing" in _err()


def test_transcript_ids_must_be_below_n_txps():
    cell_off, rp, tid, p, s, e, tl = _cells()
    bad = tid.copy()
    bad[3] = 3
    assert _call(cell_off, rp, bad, p, s, e, tl) == _lib.OEM_ERR_ARG
    assert b"n_txps" in _err()


def test_row_ptr_must_be_consistent():
    cell_off, rp, tid, p, s, e, tl = _cells()
    bad = rp.copy()
    bad[2] = 0
    assert _call(cell_off, bad, tid, p, s, e, tl) == _lib.OEM_ERR_ARG
    assert _call(cell_off, rp, tid, p, s, e, tl, nnz=5) == _lib.OEM_ERR_ARG


def test_python_wrapper_checks_its_arguments():
    cell_off, rp, tid, p, s, e, tl = _cells()
    with pytest.raises(ValueError):
        oarfish_amd.em_cells_coverage_sparse(cell_off, rp, tid, p, s, e, tl, model="kde")
    for k in range(3):   # start, end and the probabilities: one entry per alignment
        arrs = [p, s, e]
        arrs[k] = arrs[k][:-1]
        with pytest.raises(ValueError):
            oarfish_amd.em_cells_coverage_sparse(cell_off, rp, tid, arrs[0], arrs[1], arrs[2], tl)
    with pytest.raises(oarfish_amd.OemError) as ei:
        oarfish_amd.em_cells_coverage_sparse(np.array([0, 3, 2, 4], dtype=np.uint64), rp, tid, p, s, e, tl)
    assert ei.value.code == _lib.OEM_ERR_ARG
    with pytest.raises(oarfish_amd.OemError) as ei:
        oarfish_amd.em_cells_coverage_sparse(cell_off, rp, tid, p, s, e, tl, bin_width=0)
    assert ei.value.code == _lib.OEM_ERR_ARG


def test_valid_call_without_a_device_fails_loudly():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    assert _call(*_cells()) == _lib.OEM_ERR_NO_DEVICE
    cell_off, rp, tid, p, s, e, tl = _cells()
    with pytest.raises(oarfish_amd.OemError) as ei:
        oarfish_amd.em_cells_coverage_sparse(cell_off, rp, tid, p, s, e, tl, return_coverage=True)
    assert ei.value.code == _lib.OEM_ERR_NO_DEVICE
    empty = np.array([0, 0, 2, 2, 4, 4], dtype=np.uint64)   # cells without reads are valid input too
    assert _call(empty, rp, tid, p, s, e, tl) == _lib.OEM_ERR_NO_DEVICE
