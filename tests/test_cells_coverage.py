"""CPU tests of the per-cell coverage model (oem_coverage_probs_cells_device / cells_coverage_probs): every invalid
argument is refused with OEM_ERR_ARG before any device use, a valid call without a device fails with
OEM_ERR_NO_DEVICE (there is no host path behind it), and the coordinates helper of synth gives a store alignments
that lie inside their transcripts."""
import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth


def _cells():
    """Two cells of two reads each over three transcripts, with coordinates."""
    cell_off = np.array([0, 2, 4], dtype=np.uint64)
    rp = np.array([0, 1, 3, 4, 6], dtype=np.uint64)
    tid = np.array([0, 1, 2, 2, 0, 1], dtype=np.uint32)
    start = np.array([0, 10, 100, 50, 200, 0], dtype=np.uint32)
    end = np.array([300, 400, 500, 700, 600, 250], dtype=np.uint32)
    txp_len = np.array([800, 900, 1000], dtype=np.uint64)
    return cell_off, rp, tid, start, end, txp_len


def _call(cell_off, rp, tid, start, end, txp_len, n_txps=3, bin_width=100, model=1, nnz=None, out=True,
          null=None):
    nnz = len(tid) if nnz is None else nnz
    buf = np.zeros(max(len(tid), 1))
    arrs = dict(cell_row_off=cell_off, row_ptr=rp, tid=tid, start=start, end=end, txp_len=txp_len)
    ptr = {k: (None if k == null else v.ctypes.data) for k, v in arrs.items()}
    return _lib.lib().oem_coverage_probs_cells_device(
        ptr["cell_row_off"], len(cell_off) - 1, ptr["row_ptr"], ptr["tid"], ptr["start"], ptr["end"],
        ptr["txp_len"], len(rp) - 1, nnz, n_txps, bin_width, model, 2.0, 0, buf.ctypes.data if out else None)


def _err():
    return _lib.lib().oem_last_error()


def test_entry_point_is_exported():
    assert "oem_coverage_probs_cells_device" in _lib.ABI_SYMBOLS
    assert hasattr(_lib.lib(), "oem_coverage_probs_cells_device")
    assert callable(oarfish_amd.cells_coverage_probs) and "cells_coverage_probs" in oarfish_amd.__all__


@pytest.mark.parametrize("which", ["cell_row_off", "row_ptr", "tid", "start", "end", "txp_len"])
def test_null_pointers_are_refused(which):
    assert _call(*_cells(), null=which) == _lib.OEM_ERR_ARG
    assert b"NULL" in _err()


def test_null_output_is_refused():
    assert _call(*_cells(), out=False) == _lib.OEM_ERR_ARG


def test_cell_row_off_must_span_all_reads():
    cell_off, rp, tid, s, e, tl = _cells()
    assert _call(np.array([1, 2, 4], dtype=np.uint64), rp, tid, s, e, tl) == _lib.OEM_ERR_ARG
    assert b"cell_row_off" in _err()
    assert _call(np.array([0, 2, 3], dtype=np.uint64), rp, tid, s, e, tl) == _lib.OEM_ERR_ARG
    assert b"cell_row_off" in _err()


def test_cell_row_off_must_not_decrease():
    cell_off, rp, tid, s, e, tl = _cells()
    assert _call(np.array([0, 3, 2, 4], dtype=np.uint64), rp, tid, s, e, tl) == _lib.OEM_ERR_ARG
    assert b"non-decreasing" in _err()


def test_transcript_ids_must_be_below_n_txps():
    cell_off, rp, tid, s, e, tl = _cells()
    bad = tid.copy()
    bad[3] = 3
    assert _call(cell_off, rp, bad, s, e, tl) == _lib.OEM_ERR_ARG
    assert b"n_txps" in _err()


def test_row_ptr_must_be_consistent():
    cell_off, rp, tid, s, e, tl = _cells()
    bad = rp.copy()
    bad[2] = 0                                                              # decreasing
    assert _call(cell_off, bad, tid, s, e, tl) == _lib.OEM_ERR_ARG
    assert _call(cell_off, rp, tid, s, e, tl, nnz=5) == _lib.OEM_ERR_ARG     # row_ptr[n_reads] != nnz


def test_bin_width_model_and_n_txps():
    args = _cells()
    assert _call(*args, bin_width=0) == _lib.OEM_ERR_ARG
    assert b"bin width" in _err()
    for m in (-1, 2):
        assert _call(*args, model=m) == _lib.OEM_ERR_ARG
        assert b"model" in _err()
    assert _call(*args, n_txps=0) == _lib.OEM_ERR_ARG


def test_nnz_of_2_to_the_32_is_refused_without_wrapping():
    """nnz = 2^32 would wrap to 0 in a 32-bit count: it is refused before the arrays are read."""
    assert _call(*_cells(), nnz=1 << 32) == _lib.OEM_ERR_ARG
    assert b"2^32" in _err()


def test_python_wrapper_checks_its_arguments():
    cell_off, rp, tid, s, e, tl = _cells()
    with pytest.raises(ValueError):
        oarfish_amd.cells_coverage_probs(cell_off, rp, tid, s, e, tl, model="kde")
    with pytest.raises(ValueError):
        oarfish_amd.cells_coverage_probs(cell_off, rp, tid, s[:-1], e, tl)
    with pytest.raises(oarfish_amd.OemError) as ei:
        oarfish_amd.cells_coverage_probs(np.array([0, 3, 2, 4], dtype=np.uint64), rp, tid, s, e, tl)
    assert ei.value.code == _lib.OEM_ERR_ARG


def test_valid_call_without_a_device_fails_loudly():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    assert _call(*_cells()) == _lib.OEM_ERR_NO_DEVICE
    cell_off, rp, tid, s, e, tl = _cells()
    with pytest.raises(oarfish_amd.OemError) as ei:
        oarfish_amd.cells_coverage_probs(cell_off, rp, tid, s, e, tl)
    assert ei.value.code == _lib.OEM_ERR_NO_DEVICE
    # cells without reads are valid input too
    empty = np.array([0, 0, 2, 2, 4, 4], dtype=np.uint64)
    assert _call(empty, rp, tid, s, e, tl) == _lib.OEM_ERR_NO_DEVICE


def test_make_coordinates_lie_inside_their_transcripts():
    cell_off, rp, tid, p = synth.make_cells(4, 300, 80, seed=11)
    tl, s, e = synth.make_coordinates(tid, 80, zero_span_frac=0.05)
    assert tl.dtype == np.uint64 and s.dtype == e.dtype == np.uint32
    assert len(tl) == 80 and len(s) == len(e) == len(tid)
    assert np.all(s <= e) and np.all(e.astype(np.uint64) <= tl[tid])
    assert 0 < np.count_nonzero(s == e) < len(tid) // 5
    tl2, s2, e2 = synth.make_coordinates(tid, 80, zero_span_frac=0.05)
    assert np.array_equal(tl, tl2) and np.array_equal(s, s2) and np.array_equal(e, e2)   # seeded
    _, s3, e3 = synth.make_coordinates(tid, 80)
    assert np.all(e3 > s3)
