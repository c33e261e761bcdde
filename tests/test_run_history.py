"""The per-iteration rel_diff record (OEM_OPT_RUN_HISTORY, oem_run_history) without a device: the function that
turns a history into the reference's log records (em.rs:219-233 / :405-419), the declarations of the C header and of
the reference-side patch, and the entry point's argument check."""
import ctypes as C
import logging
import os
import re

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib
from oarfish_amd.em import TRACE, history_log_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [0, 9, 10, 99, 100, 1000, 1234])
def test_log_records_are_the_references_cadence(n):
    """`iteration N; rel diff R` for exactly the N % 10 == 0 up to the history's length, INFO when N % 100 == 0 and
    the level that stands for trace! otherwise, N grouped as Locale::en groups it, R = h[N - 1] as Python prints it."""
    h = np.random.default_rng(n).uniform(1e-6, 2.0, n)
    recs = history_log_records(h)
    want_n = [k for k in range(1, n + 1) if k % 10 == 0]
    assert len(recs) == len(want_n) == n // 10
    assert TRACE < logging.DEBUG
    for (level, msg), k in zip(recs, want_n):
        assert level == (logging.INFO if k % 100 == 0 else TRACE), (k, level)
        m = re.fullmatch(r"iteration ([0-9,]+); rel diff (\S+)", msg)
        assert m, msg
        assert m.group(1) == f"{k:,}" and int(m.group(1).replace(",", "")) == k
        assert float(m.group(2)) == h[k - 1] and m.group(2) == repr(float(h[k - 1]))
    by_n = {k: r for k, r in zip(want_n, recs)}
    for k in (100, 200, 1000):
        if k <= n:
            assert by_n[k][0] == logging.INFO
    if n >= 1000:
        assert by_n[1000][1].startswith("iteration 1,000; rel diff ")
        assert by_n[990][0] == TRACE and by_n[990][1].startswith("iteration 990;")
    if n >= 10:
        assert by_n[10][0] == TRACE


def _header():
    src = open(os.path.join(ROOT, "include", "oarfish_em.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_entry_point_and_the_option():
    src = _header()
    m = re.search(r"\bint\s+oem_run_history\s*\(([^)]*)\)\s*;", src)
    assert m, "oem_run_history is not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 5
    assert params[0].startswith("const oem_store") and "uint32_t run" in params[1] and "double *" in params[2]
    assert re.search(r"\bOEM_OPT_RUN_HISTORY\s*=\s*3\b", src)
    assert _lib.OEM_OPT_RUN_HISTORY == 3 and "oem_run_history" in _lib.ABI_SYMBOLS
    hpp = open(os.path.join(ROOT, "include", "oarfish_em.hpp")).read()
    assert "OEM_OPT_RUN_HISTORY" in hpp and re.search(r"std::vector<double>\s+run_history\s*\(", hpp)


def test_patch_declares_the_entry_point_with_the_headers_argument_count():
    patch = open(os.path.join(ROOT, "integration", "oarfish-mi355x.patch")).read()
    m = re.search(r"^\+\+\+ b/src/em_gpu\.rs\n@@[^\n]*\n((?:\+[^\n]*\n)+)", patch, flags=re.M)
    rs = "".join(line[1:] + "\n" for line in m.group(1).splitlines())
    block = re.search(r'unsafe extern "C" \{(.*?)\n\}', rs, flags=re.S).group(1)
    fns = dict(re.findall(r"fn (oem_[a-z0-9_]+)\s*\((.*?)\)\s*(?:->\s*[^;]+)?;", block, flags=re.S))
    assert "oem_run_history" in fns and "oem_store_set_option" in fns
    n_header = len(re.search(r"\boem_run_history\s*\(([^)]*)\)\s*;", _header()).group(1).split(","))
    assert len([p for p in fns["oem_run_history"].split(",") if p.strip()]) == n_header == 5
    # the shim logs at the reference's cadence from the record, not one closing line
    assert "oem_run_history(" in rs.split("pub fn em_gpu")[1].split("pub fn bootstrap_gpu")[0]
    assert "tracing::trace!" in rs and "Locale::en" in rs


def test_null_store_is_an_argument_error():
    L = _lib.lib()
    n = C.c_uint32(77)
    out = np.full(4, -1.0)
    assert L.oem_run_history(None, 0, out.ctypes.data, 4, C.byref(n)) == _lib.OEM_ERR_ARG
    assert b"oem_run_history" in L.oem_last_error()
    assert L.oem_run_history(None, 0, None, 0, None) == _lib.OEM_ERR_ARG
    assert n.value == 77 and np.all(out == -1.0)
    assert hasattr(oarfish_amd.DeviceStore, "run_history") and hasattr(oarfish_amd.DeviceStore, "run_history_len")
