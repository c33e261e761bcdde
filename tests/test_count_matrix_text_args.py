"""CPU tests of oem_count_matrix_text: every argument error is reported before any device use (without a device a call
that got as far as the device says OEM_ERR_NO_DEVICE), *out is NULL after any failure, and the product library exports
the entry point."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from oarfish_amd import _lib, build


def _call(cell_off, col, val, n_txps=10, row_base=0, prefix=None, prefix_len=None, n_cells=None, out=True):
    L = _lib.lib()
    h = C.c_void_p(1)
    off = None if cell_off is None else np.ascontiguousarray(cell_off, dtype=np.uint64)
    c = None if col is None else np.ascontiguousarray(col, dtype=np.uint32)
    v = None if val is None else np.ascontiguousarray(val, dtype=np.float32)
    rc = L.oem_count_matrix_text(None if off is None else off.ctypes.data, (len(off) - 1) if n_cells is None else n_cells,
                                 None if c is None else c.ctypes.data, None if v is None else v.ctypes.data, n_txps,
                                 row_base, prefix, (len(prefix) if prefix else 0) if prefix_len is None else prefix_len, 0,
                                 C.byref(h) if out else None)
    return rc, h, L


GOOD = ([0, 2, 2, 3], [0, 9, 4], [1.0, 0.5, 2.0])


@pytest.mark.parametrize("name,kw", [
    ("cell_off NULL, n_cells 3", dict(cell_off=None, col=GOOD[1], val=GOOD[2], n_cells=3)),
    ("col NULL with entries", dict(cell_off=GOOD[0], col=None, val=GOOD[2])),
    ("val NULL with entries", dict(cell_off=GOOD[0], col=GOOD[1], val=None)),
    ("cell_off[0] != 0", dict(cell_off=[1, 2, 2, 3], col=GOOD[1], val=GOOD[2])),
    ("cell_off decreasing", dict(cell_off=[0, 2, 1, 3], col=GOOD[1], val=GOOD[2])),
    ("col == n_txps", dict(cell_off=GOOD[0], col=[0, 10, 4], val=GOOD[2])),
    ("col above n_txps", dict(cell_off=GOOD[0], col=[0, 9, 2 ** 32 - 1], val=GOOD[2])),
    ("row_base + n_cells = 2^32", dict(cell_off=GOOD[0], col=GOOD[1], val=GOOD[2], row_base=2 ** 32 - 3)),
    ("prefix NULL with a length", dict(cell_off=GOOD[0], col=GOOD[1], val=GOOD[2], prefix=None, prefix_len=4)),
])
def test_argument_errors_come_before_the_device(name, kw):
    rc, h, L = _call(**kw)
    assert rc == _lib.OEM_ERR_ARG, name
    assert h.value is None and b"oem_count_matrix_text" in L.oem_last_error()


def test_null_out_is_an_argument_error():
    rc, _, _ = _call(*GOOD, out=False)
    assert rc == _lib.OEM_ERR_ARG


def test_a_valid_call_needs_a_device():
    """row_base + n_cells = 2^32 - 1 is the largest legal; with no device the answer is OEM_ERR_NO_DEVICE (there is no
    host fallback), with one the call succeeds."""
    for kw in (dict(), dict(row_base=2 ** 32 - 4), dict(prefix=b"%%x\n"), dict(cell_off=[0], col=None, val=None)):
        args = dict(cell_off=GOOD[0], col=GOOD[1], val=GOOD[2])
        args.update(kw)
        rc, h, L = _call(**args)
        if _lib.device_count() > 0:
            assert rc == _lib.OEM_OK and h.value is not None
            L.oem_text_result_destroy(h)
        else:
            assert rc == _lib.OEM_ERR_NO_DEVICE and h.value is None


def test_python_wrapper_checks_its_own_arguments():
    from oarfish_amd.em import count_matrix_text
    with pytest.raises(ValueError):
        count_matrix_text([0, 2], [1], [1.0], 10)
    with pytest.raises(ValueError):
        count_matrix_text([0, 1], [1], [1.0, 2.0], 10)
    with pytest.raises(_lib.OemError) as ei:
        count_matrix_text([0, 1], [10], [1.0], 10)
    assert ei.value.code == _lib.OEM_ERR_ARG


def test_the_product_library_exports_the_symbol():
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB_PATH], text=True)
    assert "oem_count_matrix_text" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "oem_count_matrix_text" in build.header_symbols()
