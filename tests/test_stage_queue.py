"""The staging queue of the records and barcoded cells sessions (oarfish_amd/csrc/oem_stage_queue.h), without a device:
tests/native/stage_queue_main.cpp runs the protocol -- tickets, budget, pool, allocator failure, status errors, close and
cancel -- with a counting allocator, once under ThreadSanitizer and once under AddressSanitizer + UBSan."""
import os
import platform
import re
import shutil
import subprocess

import pytest

from oarfish_amd import build as _b

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "stage_queue_main.cpp")
CSRC = os.path.join(ROOT, "oarfish_amd", "csrc")
HDR = os.path.join(CSRC, "oem_stage_queue.h")
SCENARIOS = ["ticket order and payload", "oversized batch", "allocator failure 1", "allocator failure 2", "status error while blocked",
             "push in flight", "close", "cancel", "pool"]


@pytest.mark.parametrize("name,sanitize", [("tsan", "thread"), ("asan", "address,undefined")])
def test_the_protocol_under_sanitizers(name, sanitize):
    exe = os.path.join(HERE, "native", "stage_queue_main_" + name)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread", "-fsanitize=" + sanitize,
                               "-fno-sanitize-recover=all", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    if r.returncode != 0 and "unexpected memory mapping" in r.stderr and shutil.which("setarch"):
        # ThreadSanitizer's runtime gives up before main() where the kernel randomises mappings over more bits than its
        # shadow layout knows: the same program, started without address-space randomisation
        r = subprocess.run(["setarch", platform.machine(), "-R", exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr[-3000:])
    assert r.stdout.splitlines() == ["ok " + s for s in SCENARIOS]
    assert "Sanitizer" not in r.stderr, r.stderr[-3000:]


def _code(path):
    """The file without its comments."""
    src = open(path).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def test_the_header_is_host_only_and_the_sessions_keep_no_copy_of_the_protocol():
    hdr = _code(HDR)
    assert "hip" not in hdr.lower()
    assert [i for i in re.findall(r'#include\s+"([^"]+)"', hdr)] == []           # the standard library and nothing else
    assert "oem_stage_queue.h" in _b.HEADERS
    records = _code(os.path.join(CSRC, "oem_records_stream.hip"))
    barcodes = _code(os.path.join(CSRC, "oem_cells_barcodes_stream.hip"))
    assert "condition_variable" not in records
    assert re.findall(r"std::condition_variable\s+([^;]+);", barcodes) == ["cv_groups"]   # the group hand-off only
    for src in (records, barcodes):
        assert "StageQueue<Batch>" in src and "struct Batch : StageBatch" in src
        assert "hipHostMalloc" not in src and "cv_space" not in src and "pushes_in_flight = " not in src
    # one definition of "page-lock on this device, else malloc" for the two sessions
    sources = [f for f in os.listdir(CSRC) if os.path.isfile(os.path.join(CSRC, f))]
    uses = [f for f in sources if "hipHostMallocPortable" in _code(os.path.join(CSRC, f))]
    assert sorted(uses) == ["oem_cells_stream.hip", "oem_parse_device.h"]
    assert sum(_code(os.path.join(CSRC, f)).count("struct U32AsU64") for f in sources) == 1
