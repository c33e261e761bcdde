"""The bulk records session (oem_records_stream_*) without a device: oem_records_stream_create reports every argument
error before any device use, and without a device it fails with OEM_ERR_NO_DEVICE.  The session itself is held to the
one call in tests/test_records_stream_gpu.py; that the header still compiles as C99 and that the exports equal it is
tests/test_abi.py's."""
import ctypes as C

import numpy as np
import pytest

from oarfish_amd import _lib
from oarfish_amd.builder import filters_c
from oracle import filter_py as fp

from tests.filter_common import filters_dict


def _create(L, opts, filters, txp_len):
    h = C.c_void_p(1)                                                  # (a failing call has to clear it)
    rc = L.oem_records_stream_create(C.byref(opts) if opts is not None else None,
                                     C.addressof(filters) if filters is not None else None,
                                     txp_len.ctypes.data if txp_len is not None else None, C.byref(h))
    return rc, h, (L.oem_last_error() or b"").decode()


def _opts(n_txps=2, model=-1, bin_width=100, reserved=(0, 0, 0, 0), device=0):
    o = _lib.RecordsStreamOptsC()
    o.n_txps, o.device, o.bin_width, o.model, o.growth_rate, o.max_staged_records = n_txps, device, bin_width, model, 2.0, 0
    for k, v in enumerate(reserved):
        o.reserved[k] = v
    return o


def test_opts_structure_is_the_headers():
    assert C.sizeof(_lib.RecordsStreamOptsC) == 48                     # 4 x 4, f64, u64, 4 x 4: no padding
    assert _lib.RecordsStreamOptsC.growth_rate.offset == 16 and _lib.RecordsStreamOptsC.reserved.offset == 32


@pytest.mark.parametrize("what", ["opts", "filters", "txp_len", "n_txps", "model low", "model high", "bin_width",
                                  "reserved 0", "reserved 3"])
def test_create_reports_argument_errors_before_any_device_use(what):
    """every one of these is OEM_ERR_ARG with and without a device: the checks come first"""
    L = _lib.lib()
    F = filters_c(filters_dict(fp.Filters()))
    tl = np.array([1000, 2000], dtype=np.uint64)
    o = {"n_txps": _opts(n_txps=0), "model low": _opts(model=-2), "model high": _opts(model=2),
         "bin_width": _opts(model=0, bin_width=0), "reserved 0": _opts(reserved=(1, 0, 0, 0)),
         "reserved 3": _opts(reserved=(0, 0, 0, 7))}.get(what, _opts())
    o.device = 10 ** 6                                                 # (no such device: it is never asked for)
    rc, h, msg = _create(L, None if what == "opts" else o, None if what == "filters" else F, None if what == "txp_len" else tl)
    assert rc == _lib.OEM_ERR_ARG and not h.value, msg
    assert "oem_records_stream_create" in msg or "bin width" in msg


def test_create_out_null_and_bin_width_without_a_model():
    L = _lib.lib()
    F = filters_c(filters_dict(fp.Filters()))
    tl = np.array([1000, 2000], dtype=np.uint64)
    o = _opts()
    assert L.oem_records_stream_create(C.byref(o), C.addressof(F), tl.ctypes.data, None) == _lib.OEM_ERR_ARG
    if _lib.device_count() == 0:                                       # bin_width = 0 without a model is no error
        rc, h, _ = _create(L, _opts(bin_width=0), F, tl)
        assert rc == _lib.OEM_ERR_NO_DEVICE and not h.value


def test_create_without_a_device_fails_loudly():
    if _lib.device_count() > 0:
        L = _lib.lib()                                                 # with one: the session exists and can be dropped
        rc, h, msg = _create(L, _opts(), filters_c(filters_dict(fp.Filters())), np.array([1000, 2000], dtype=np.uint64))
        assert rc == _lib.OEM_OK and h.value, msg
        L.oem_records_stream_destroy(h)
        return
    L = _lib.lib()
    for model in (-1, 0, 1):
        rc, h, msg = _create(L, _opts(model=model), filters_c(filters_dict(fp.Filters())), np.array([1000, 2000], dtype=np.uint64))
        assert rc == _lib.OEM_ERR_NO_DEVICE and not h.value, msg


def test_destroy_null_is_a_no_op_and_null_sessions_are_argument_errors():
    L = _lib.lib()
    L.oem_records_stream_destroy(None)
    v, t, h = C.c_uint64(0), C.c_uint64(0), C.c_void_p(1)
    off = np.zeros(1, dtype=np.uint64)
    assert L.oem_records_stream_info(None, _lib.OEM_RECORDS_STREAM_INFO_BATCHES, C.byref(v)) == _lib.OEM_ERR_ARG
    assert L.oem_records_stream_push(None, None, off.ctypes.data, 0, C.byref(t)) == _lib.OEM_ERR_ARG
    assert L.oem_records_stream_finish(None, None, None, None, C.byref(h)) == _lib.OEM_ERR_ARG and not h.value
