"""CPU tests of the bulk coverage model + store creation in one call (oem_store_create_coverage,
oem_builder_store_create_coverage, DeviceStore.with_coverage): both entry points are exported and declared, every
invalid argument is refused with OEM_ERR_ARG and the composition's message before any device use, a valid call
without a device fails with OEM_ERR_NO_DEVICE, and the Python wrappers check their own arguments."""
import ctypes as C
import os

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, bulk

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "oarfish_em.h")


def _store():
    """Three reads over three transcripts, with probabilities and coordinates."""
    rp = np.array([0, 1, 3, 6], dtype=np.uint64)
    tid = np.array([0, 1, 2, 2, 0, 1], dtype=np.uint32)
    p = np.array([1.0, 0.5, 0.5, 1.0, 0.3, 0.7], dtype=np.float32)
    start = np.array([0, 10, 100, 50, 200, 0], dtype=np.uint32)
    end = np.array([300, 400, 500, 700, 600, 250], dtype=np.uint32)
    txp_len = np.array([800, 900, 1000], dtype=np.uint64)
    return rp, tid, p, start, end, txp_len


def _call(rp, tid, p, start, end, txp_len, n_txps=3, bin_width=100, model=0, nnz=None, n_reads=None, null=None,
          out=True, cov=False, **opts):
    nnz = len(tid) if nnz is None else nnz
    n_reads = len(rp) - 1 if n_reads is None else n_reads
    arrs = dict(row_ptr=rp, tid=tid, p=p, start=start, end=end, txp_len=txp_len)
    ptr = {k: (None if k == null else v.ctypes.data) for k, v in arrs.items()}
    o = _lib.StoreOptsC()
    for k, v in opts.items():
        setattr(o, k, v)
    col = np.empty(len(tid))
    h = C.c_void_p()
    rc = _lib.lib().oem_store_create_coverage(
        ptr["row_ptr"], ptr["tid"], ptr["p"], ptr["start"], ptr["end"], ptr["txp_len"], n_reads, nnz, n_txps,
        bin_width, model, 2.0, 0, C.addressof(o), col.ctypes.data if cov else None, C.byref(h) if out else None)
    if h.value:
        _lib.lib().oem_store_destroy(h)
    if rc != _lib.OEM_OK and out:
        assert not h.value, "a failed call returned a store"
    return rc


def _err():
    return _lib.lib().oem_last_error()


def test_entry_points_are_exported_and_declared():
    with open(HEADER) as f:
        header = f.read()
    for name in ("oem_store_create_coverage", "oem_builder_store_create_coverage"):
        assert name in _lib.ABI_SYMBOLS
        assert hasattr(_lib.lib(), name)
        assert f"int {name}(" in header
    assert callable(oarfish_amd.DeviceStore.with_coverage)
    assert callable(oarfish_amd.InMemoryAlignmentStore.model_coverage_on_device)


@pytest.mark.parametrize("which", ["row_ptr", "tid", "p", "start", "end", "txp_len"])
def test_null_pointers_are_refused(which):
    assert _call(*_store(), null=which) == _lib.OEM_ERR_ARG
    assert b"oem_store_create_coverage: NULL argument" in _err()


def test_null_result_handle_is_refused():
    assert _call(*_store(), out=False) == _lib.OEM_ERR_ARG
    assert b"out is NULL" in _err()


def test_bin_width_model_and_n_txps():
    args = _store()
    assert _call(*args, bin_width=0) == _lib.OEM_ERR_ARG
    assert b"coverage model with 0 bin width is not implemented" in _err()
    for m in (-1, 2):
        assert _call(*args, model=m) == _lib.OEM_ERR_ARG
        assert b"model must be 0 (logistic) or 1 (binomial)" in _err()
    assert _call(*args, n_txps=0) == _lib.OEM_ERR_ARG
    assert b"n_txps is 0" in _err()


def test_nnz_of_2_to_the_32_is_refused_without_wrapping():
    assert _call(*_store(), nnz=1 << 32) == _lib.OEM_ERR_ARG
    assert b"needs nnz < 2^32" in _err()


def test_row_ptr_must_span_all_alignments_and_not_decrease():
    rp, tid, p, s, e, tl = _store()
    assert _call(rp, tid, p, s, e, tl, nnz=5) == _lib.OEM_ERR_ARG
    assert b"row_ptr must span [0, nnz]" in _err()
    assert _call(np.array([1, 1, 3, 6], dtype=np.uint64), tid, p, s, e, tl) == _lib.OEM_ERR_ARG
    assert b"row_ptr must span [0, nnz]" in _err()
    assert _call(np.array([0, 4, 3, 6], dtype=np.uint64), tid, p, s, e, tl) == _lib.OEM_ERR_ARG
    assert b"row_ptr is not non-decreasing at read 1" in _err()


def test_transcript_ids_must_be_below_n_txps():
    rp, tid, p, s, e, tl = _store()
    bad = tid.copy()
    bad[4] = 3
    assert _call(rp, bad, p, s, e, tl) == _lib.OEM_ERR_ARG
    assert b"tid[4]=3 is not below n_txps=3" in _err()


@pytest.mark.parametrize("field,value,msg", [("weight_coding", 3, b"weight_coding 3 (0, 1 or 2)"),
                                             ("layout_build", 2, b"layout_build 2 (0 or 1)"),
                                             ("reorder_rows", 3, b"reorder_rows 3 (0, 1 or 2)")])
def test_store_options_out_of_range(field, value, msg):
    assert _call(*_store(), **{field: value}) == _lib.OEM_ERR_ARG
    assert msg in _err()


def test_builder_variant_checks_its_builder():
    h = C.c_void_p(1)
    assert _lib.lib().oem_builder_store_create_coverage(None, 100, 0, 2.0, 0, None, None, C.byref(h)) == _lib.OEM_ERR_ARG
    assert not h.value
    assert b"builder is NULL" in _err()


def test_valid_call_without_a_device_fails_loudly():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    for wc in (0, 1, 2):
        assert _call(*_store(), weight_coding=wc) == _lib.OEM_ERR_NO_DEVICE
    assert _call(*_store(), cov=True, layout_build=1, reorder_rows=2) == _lib.OEM_ERR_NO_DEVICE
    rp, tid, p, s, e, tl = _store()
    with pytest.raises(oarfish_amd.OemError) as ei:
        oarfish_amd.DeviceStore.with_coverage(rp, tid, p, s, e, tl, return_coverage=True)
    assert ei.value.code == _lib.OEM_ERR_NO_DEVICE
    st = oarfish_amd.InMemoryAlignmentStore.from_arrays(rp, tid, p)
    with pytest.raises(oarfish_amd.OemError):
        st.model_coverage_on_device(s, e, tl)
    assert not st.filter_opts.model_coverage   # nothing changes on failure


def test_python_wrappers_check_their_arguments():
    rp, tid, p, s, e, tl = _store()
    with pytest.raises(ValueError):
        oarfish_amd.DeviceStore.with_coverage(rp, tid, p, s, e, tl, model="kde")
    for k in range(3):   # probabilities, start and end: one entry per alignment
        arrs = [p, s, e]
        arrs[k] = arrs[k][:-1]
        with pytest.raises(ValueError):
            oarfish_amd.DeviceStore.with_coverage(rp, tid, arrs[0], arrs[1], arrs[2], tl)
    with pytest.raises(oarfish_amd.OemError) as ei:
        oarfish_amd.DeviceStore.with_coverage(rp, tid, p, s, e, tl, bin_width=0)
    assert ei.value.code == _lib.OEM_ERR_ARG
    with pytest.raises(oarfish_amd.OemError) as ei:
        oarfish_amd.DeviceStore.with_coverage(rp, tid, p, s, e, tl, weight_coding=3)
    assert ei.value.code == _lib.OEM_ERR_ARG
    st = oarfish_amd.InMemoryAlignmentStore.from_arrays(rp, tid, p)
    with pytest.raises(ValueError):
        st.model_coverage_on_device(s[:-1], e, tl)
    cov = bulk.BulkCoverage(s, e)
    assert cov.bin_width == 100 and cov.growth_rate == 2.0
