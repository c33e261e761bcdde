"""CPU tests of the per-cell session's C ABI (oem_cells_stream_*): declared, exported, bound, and its argument
errors come before any device use."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from oarfish_amd import _lib
from oarfish_amd import build as _b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["oem_cells_stream_create", "oem_cells_stream_push", "oem_cells_stream_finish", "oem_cells_stream_info",
                "oem_cells_stream_destroy"]


def _opts(**kw):
    o = _lib.CellsStreamOptsC()
    o.n_txps, o.device, o.max_iter, o.conv_thresh = 10, 0, 100, 1e-3
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "oarfish_em.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(oem_[a-z0-9_]+)\s*\(", src))
    out = subprocess.check_output(["nm", "-D", "--defined-only", _b.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert name in exported, name
        assert name in _lib.ABI_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    assert "oem_cells_stream_opts" in src and "typedef struct oem_cells_stream oem_cells_stream;" in src
    assert L.oem_abi_version() == 2


def test_opts_struct_matches_the_header(tmp_path):
    """The ctypes mirror of oem_cells_stream_opts has the C compiler's size and field offsets."""
    fields = [f[0] for f in _lib.CellsStreamOptsC._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "oarfish_em.h"\nint main(void) {\n'
    prog += '  printf("%zu\\n", sizeof(oem_cells_stream_opts));\n'
    for f in fields:
        prog += f'  printf("%zu\\n", offsetof(oem_cells_stream_opts, {f}));\n'
    prog += "  return 0;\n}\n"
    src, exe = tmp_path / "opts.c", tmp_path / "opts"
    src.write_text(prog)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [C.sizeof(_lib.CellsStreamOptsC)] + [getattr(_lib.CellsStreamOptsC, f).offset for f in fields]
    assert got == want


def test_create_reports_argument_errors_before_any_device_use():
    L = _lib.lib()
    tl = np.full(10, 1000, dtype=np.uint64)
    cases = [
        (_opts(n_txps=0), None, b"n_txps"),
        (_opts(coverage=1, bin_width=100, model=1), None, b"txp_len"),
        (_opts(coverage=1, bin_width=0, model=1), tl, b"bin width"),
        (_opts(coverage=1, bin_width=100, model=2), tl, b"model"),
        (_opts(coverage=2), None, b"coverage"),
    ]
    for o, t, word in cases:
        h = C.c_void_p(1)
        rc = L.oem_cells_stream_create(C.byref(o), None if t is None else t.ctypes.data, C.byref(h))
        assert rc == _lib.OEM_ERR_ARG and word in L.oem_last_error(), (word, rc, L.oem_last_error())
        assert not h.value
    o = _opts()
    o.reserved[2] = 1
    h = C.c_void_p(1)
    assert L.oem_cells_stream_create(C.byref(o), None, C.byref(h)) == _lib.OEM_ERR_ARG and not h.value
    assert L.oem_cells_stream_create(None, None, C.byref(h)) == _lib.OEM_ERR_ARG
    assert L.oem_cells_stream_create(C.byref(_opts()), None, None) == _lib.OEM_ERR_ARG


def test_create_without_a_device_is_no_device():
    """A valid create needs a device: none here means OEM_ERR_NO_DEVICE and no handle (with a device: a session)."""
    L = _lib.lib()
    h = C.c_void_p(1)
    rc = L.oem_cells_stream_create(C.byref(_opts()), None, C.byref(h))
    if _lib.device_count() > 0:
        assert rc == _lib.OEM_OK and h.value
        L.oem_cells_stream_destroy(h)
    else:
        assert rc == _lib.OEM_ERR_NO_DEVICE and not h.value
        import oarfish_amd
        try:
            oarfish_amd.CellsStream(10)
        except oarfish_amd.OemError as e:
            assert e.code == _lib.OEM_ERR_NO_DEVICE
        else:
            raise AssertionError("CellsStream without a device must raise")


def test_null_handles():
    L = _lib.lib()
    L.oem_cells_stream_destroy(None)   # a no-op
    rp = np.zeros(1, dtype=np.uint64)
    assert L.oem_cells_stream_push(None, rp.ctypes.data, None, None, None, None, 0, 0, None) == _lib.OEM_ERR_ARG
    res = C.c_void_p(1)
    assert L.oem_cells_stream_finish(None, C.byref(res)) == _lib.OEM_ERR_ARG and not res.value
    v = C.c_uint64(0)
    assert L.oem_cells_stream_info(None, 1, C.byref(v)) == _lib.OEM_ERR_ARG
