"""The growth rule and the allocation sizes of the sessions' device arena (oarfish_amd/csrc/oem_dev_blob.h), without a
device: tests/native/dev_blob_main.cpp checks next_cap and the sizes derived from a capacity under AddressSanitizer +
UBSan.  The device side runs in tests/test_session_arena_growth_gpu.py."""
import os
import re
import subprocess

from oarfish_amd import build as _b

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "dev_blob_main.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "oarfish_amd", "csrc")
HDR = os.path.join(CSRC, "oem_dev_blob.h")
SCENARIOS = ["need against twice the capacity", "the first capacity with each floor", "need of 0", "floors of 1", "allocation sizes"]


def test_next_cap_and_the_allocation_sizes_under_sanitizers():
    exe = os.path.join(HERE, "native", "dev_blob_main")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr[-3000:])
    assert r.stdout.splitlines() == ["ok " + s for s in SCENARIOS]
    assert "Sanitizer" not in r.stderr, r.stderr[-3000:]


def _code(path):
    """The file without its comments."""
    src = open(path).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def test_the_sessions_keep_no_copy_of_the_arena():
    assert "oem_dev_blob.h" in _b.HEADERS and "oem_dev_blob.hip" in _b.SOURCES
    sessions = [_code(os.path.join(CSRC, f)) for f in ("oem_records_stream.hip", "oem_cells_barcodes_stream.hip", "oem_cells_barcodes_sort_stream.hip")]
    for src in sessions:
        for gone in ("struct SortArena", "struct Arena", "k_offsets_shift", "k_barcode_label_offsets", "k_global_index", "k_arena_append",
                     "ref_check(uint64_t"):
            assert gone not in src, gone
    sources = [f for f in os.listdir(CSRC) if os.path.isfile(os.path.join(CSRC, f))]
    for once in ("void k_records_ref_check", "void k_offsets_rebase", "void k_survivor_append", "uint64_t next_cap"):
        assert sum(_code(os.path.join(CSRC, f)).count(once) for f in sources) == 1, once
