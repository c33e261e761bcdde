"""CPU tests of Rust's `{}` for an f64 (oarfish_amd/csrc/oem_shortest_f64.h) and of the two entry points that print
with it (oem_quant_text, oem_ambig_text), as far as they go without a device.

The header's pure functions -- the ones the kernels of oem_quant_text.hip call -- are checked twice.  A stand-alone
host program with the address and undefined-behaviour sanitizers on (tests/native/shortest_f64_main.cpp) holds them,
without any reference of this project's, to strtod, to shortness, to std::to_chars and to the header's own bound on the
length; it gives each text a heap block of exactly the measured length, so a printer that writes one byte more than
it measured is a sanitizer report.  And through the test-only library's host hook (oem_test_shortest_f64) the same
functions are held to `writers.rust_display`, the formatting of the `.quant` writer the device form replaces."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oarfish_amd import _lib, build
from oarfish_amd.writers import rust_display

from .shortest_f64_common import LONGEST, as_f64, bits_of, edge_bits, seeded_bits

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "shortest_f64_main.cpp")
EXE = os.path.join(HERE, "native", "shortest_f64_main")
CSRC = os.path.join(HERE, "..", "oarfish_amd", "csrc")
HDRS = [os.path.join(CSRC, "oem_shortest_f64.h"), os.path.join(CSRC, "oem_text_format.h")]
N_RANDOM = 1_000_000


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-o", EXE, SRC])
    return EXE


def header_max_len() -> int:
    """kShortestF64MaxLen as the header derives it: 1 + 2 + the table's greatest decimal exponent."""
    hdr = open(HDRS[0]).read()
    assert "constexpr uint32_t kShortestF64MaxLen = 1 + 2 + (uint32_t)kSf64Pow10Max;" in hdr
    return 3 + int(re.search(r"kSf64Pow10Max = (\d+);", hdr).group(1))


def test_self_checks_of_the_stand_alone_program(exe):
    """Every power of two and of ten with its neighbours, the subnormal edge, DBL_MAX, 2^53 +- 1, 0.1 + 0.2, 1e21 ..
    1e23, the zeros, published hard cases and 10^6 random bit patterns: strtod reads every text back; one digit fewer
    never does; the digits are std::to_chars'; the measured length is the emitted one; the longest text is the header's
    bound."""
    r = subprocess.run([exe, "--sweep", str(N_RANDOM), "20250118"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    f = r.stdout.split()
    assert f[0] == "checked" and int(f[1]) >= N_RANDOM + 8000, r.stdout
    assert int(f[3]) == int(f[5]) == header_max_len() == 327


def test_stand_alone_program_prints_the_fixed_texts(exe):
    bits = bits_of([1.0, 0.1, 1e23, -0.0, 0.0, 5e-324]).tolist() + [LONGEST]
    r = subprocess.run([exe], input="".join(f"{b:x}\n" for b in bits), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    tiny = "0." + "0" * 323 + "5"
    assert r.stdout.split("\n")[:-1] == ["1 1", "0.1 3", "1" + "0" * 23 + " 24", "-0 2", "0 1", f"{tiny} 326", f"-{tiny} 327"]


def host_texts(bits):
    """The header's text of every pattern, through the test-only library's host hook."""
    L = _lib.testing_lib()
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    cap = 327 * len(bits)
    text = np.zeros(max(cap, 1), dtype=np.uint8)
    off = np.zeros(len(bits) + 1, dtype=np.uint64)
    rc = L.oem_test_shortest_f64(bits.ctypes.data, len(bits), text.ctypes.data, cap, off.ctypes.data)
    assert rc == _lib.OEM_OK, L.oem_last_error()
    raw = text.tobytes()
    return [raw[int(a):int(b)].decode() for a, b in zip(off[:-1], off[1:])]


def check_against_rust_display(bits):
    got = host_texts(bits)
    for b, x, t in zip(bits, as_f64(bits), got):
        assert t == rust_display(x), (hex(int(b)), t)


def test_edge_list_equals_rust_display():
    bits = edge_bits()
    assert len(bits) > 8000
    check_against_rust_display(bits)
    assert host_texts([LONGEST])[0] == "-0." + "0" * 323 + "5"


def test_seeded_values_equal_rust_display():
    """10^5 values: random finite bit patterns, and counts as an EM leaves them (log-uniform, integers, eighths)."""
    bits = seeded_bits()
    assert len(bits) == 100_000
    check_against_rust_display(bits)


def test_host_hook_refuses_a_value_that_is_not_finite():
    L = _lib.testing_lib()
    bits = bits_of([1.0, np.inf])
    text, off = np.zeros(700, dtype=np.uint8), np.zeros(3, dtype=np.uint64)
    assert L.oem_test_shortest_f64(bits.ctypes.data, 2, text.ctypes.data, 700, off.ctypes.data) == _lib.OEM_ERR_ARG


def test_table_is_the_generated_one():
    gen = os.path.join(HERE, "..", "scripts", "gen_shortest_f64_table.py")
    assert subprocess.run([sys.executable, gen, "--check"]).returncode == 0


# -- the entry points without a device ---------------------------------------------------------------------------------
def _quant(names=(b"a", b"bc"), lens=(1, 2), counts=(1.0, 0.5), name_off=None, n=None, prefix=None, prefix_len=None,
           out=True, null=()):
    L = _lib.lib()
    h = C.c_void_p(1)
    blob = np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8)
    off = np.zeros(len(names) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in names])
    if name_off is not None:
        off = np.asarray(name_off, dtype=np.uint64)
    ln = np.asarray(lens, dtype=np.uint64)
    ct = np.asarray(counts, dtype=np.float64)
    ptr = {"names": blob, "name_off": off, "lens": ln, "counts": ct}
    a = [None if k in null else v.ctypes.data for k, v in ptr.items()]
    rc = L.oem_quant_text(a[0], a[1], a[2], a[3], len(names) if n is None else n, prefix,
                          (len(prefix) if prefix else 0) if prefix_len is None else prefix_len, 0,
                          C.byref(h) if out else None)
    return rc, h, L


def _ambig(unique=(1, 2), total=(3, 4), n=None, prefix=None, prefix_len=None, out=True, null=()):
    L = _lib.lib()
    h = C.c_void_p(1)
    u, t = np.asarray(unique, dtype=np.uint32), np.asarray(total, dtype=np.uint32)
    rc = L.oem_ambig_text(None if "unique" in null else u.ctypes.data, None if "total" in null else t.ctypes.data,
                          len(u) if n is None else n, prefix, (len(prefix) if prefix else 0) if prefix_len is None else prefix_len,
                          0, C.byref(h) if out else None)
    return rc, h, L


@pytest.mark.parametrize("name,kw", [
    ("a count that is NaN", dict(counts=(1.0, float("nan")))),
    ("a count that is +inf", dict(counts=(float("inf"), 1.0))),
    ("a count that is -inf", dict(counts=(1.0, float("-inf")))),
    ("name_off decreasing", dict(name_off=[0, 2, 1])),
    ("a name with a tab", dict(names=(b"a", b"b\tc"))),
    ("a name with a newline", dict(names=(b"a\n", b"bc"))),
    ("names NULL", dict(null=("names",))),
    ("name_off NULL", dict(null=("name_off",))),
    ("lens NULL", dict(null=("lens",))),
    ("counts NULL", dict(null=("counts",))),
    ("prefix NULL with a length", dict(prefix=None, prefix_len=4)),
])
def test_quant_text_argument_errors_come_before_the_device(name, kw):
    rc, h, L = _quant(**kw)
    assert rc == _lib.OEM_ERR_ARG, name
    assert h.value is None and b"oem_quant_text" in L.oem_last_error()


@pytest.mark.parametrize("name,kw", [
    ("unique NULL", dict(null=("unique",))),
    ("total NULL", dict(null=("total",))),
    ("prefix NULL with a length", dict(prefix=None, prefix_len=1)),
])
def test_ambig_text_argument_errors_come_before_the_device(name, kw):
    rc, h, L = _ambig(**kw)
    assert rc == _lib.OEM_ERR_ARG, name
    assert h.value is None and b"oem_ambig_text" in L.oem_last_error()


def test_null_out_is_an_argument_error():
    assert _quant(out=False)[0] == _lib.OEM_ERR_ARG
    assert _ambig(out=False)[0] == _lib.OEM_ERR_ARG


def test_a_valid_call_needs_a_device():
    """With no device the answer is OEM_ERR_NO_DEVICE (there is no host fallback), also for no transcripts at all (NULL
    arrays are fine then); with one the call succeeds."""
    calls = [lambda: _quant(), lambda: _quant(prefix=b"tname\tlen\tnum_reads\n"),
             lambda: _quant(names=(), lens=(), counts=(), null=("names", "name_off", "lens", "counts")),
             lambda: _quant(counts=(-0.0, 5e-324)),
             lambda: _ambig(), lambda: _ambig(unique=(5,), total=(2,)),
             lambda: _ambig(unique=(), total=(), null=("unique", "total"), prefix=b"x\n")]
    for call in calls:
        rc, h, L = call()
        if _lib.device_count() > 0:
            assert rc == _lib.OEM_OK and h.value is not None
            L.oem_text_result_destroy(h)
        else:
            assert rc == _lib.OEM_ERR_NO_DEVICE and h.value is None


def test_python_wrappers_check_their_own_arguments():
    from oarfish_amd import writers
    with pytest.raises(ValueError):
        writers.quant_text(["a", "b"], [1], [1.0, 2.0])
    with pytest.raises(ValueError):
        writers.ambig_text([1, 2], [1])
    with pytest.raises(ValueError):
        writers.write_output_device("unused", {}, ["a"], [1], [1.0], ([1, 2], [1, 2]))
    with pytest.raises(_lib.OemError) as ei:
        writers.quant_text(["a", "b"], [1, 2], [1.0, float("nan")])
    assert ei.value.code == _lib.OEM_ERR_ARG


def test_pack_names():
    from oarfish_amd.writers import pack_names
    for names in (["ab", "", "cde", "éx"], [b"ab", "c"], ["a\nb", "c"], [], [""], ["", ""]):
        blob, off = pack_names(names)
        enc = [x.encode() if isinstance(x, str) else x for x in names]
        assert blob.tobytes() == b"".join(enc) and off.tolist() == np.cumsum([0] + [len(x) for x in enc]).tolist()


def test_the_product_library_exports_the_symbols():
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for sym in ("oem_quant_text", "oem_ambig_text"):
        assert sym in exported and sym in build.header_symbols() and sym in _lib.ABI_SYMBOLS
    assert "oem_test_shortest_f64" not in exported
