"""CPU tests of the oem_assignment_text entry points: argument errors come before any device use, the result calls
take NULL as documented, and the Python helpers pack read names the way the C ABI takes them."""
import ctypes as C

import numpy as np
import pytest

from oarfish_amd import _lib
from oarfish_amd.types import pack_read_names


def test_null_arguments_are_argument_errors_not_device_errors():
    L = _lib.lib()
    counts = np.ones(3)
    h = C.c_void_p(1)
    # (without a device a call that got as far as the device would say OEM_ERR_NO_DEVICE)
    assert L.oem_assignment_text(None, counts.ctypes.data, 1e-3, None, None, C.byref(h)) == _lib.OEM_ERR_ARG
    assert h.value is None and b"oem_assignment_text" in L.oem_last_error()
    assert L.oem_assignment_text(None, None, 1e-3, None, None, None) == _lib.OEM_ERR_ARG
    L.oem_text_result_destroy(None)
    assert L.oem_text_result_dims(None, None, None, None) == _lib.OEM_ERR_ARG
    assert L.oem_text_result_copy(None, None, None, None) == _lib.OEM_ERR_ARG


def test_pack_read_names():
    blob, off = pack_read_names(["ab", b"c\0", "", "dé"], 4)
    assert blob.tobytes() == b"abc\0d\xc3\xa9" and list(off) == [0, 2, 4, 4, 7] and off.dtype == np.uint64
    b2, o2 = pack_read_names((blob, off), 4)
    assert b2.tobytes() == blob.tobytes() and np.array_equal(o2, off)
    b3, _ = pack_read_names((blob.tobytes(), list(off)), 4)
    assert b3.tobytes() == blob.tobytes()
    with pytest.raises(ValueError):
        pack_read_names(["a"], 2)
    with pytest.raises(ValueError):
        pack_read_names((blob, off[:-1]), 4)
    with pytest.raises(ValueError):
        pack_read_names((blob[:3], off), 4)
    blob0, off0 = pack_read_names([], 0)
    assert len(blob0) == 0 and list(off0) == [0]
