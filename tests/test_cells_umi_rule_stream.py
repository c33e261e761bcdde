"""The UMI rule in the barcoded sessions, without a device (oem_cells_stream_set_umi_rule, oem_cells_stream_umi_rule_copy):
the ABI's shape, the errors that precede device use, the wrapper's and the driver's own checks.
tests/test_cells_umi_rule_stream_gpu.py holds the sessions to the rule one call and to the join, and checks the state
errors that need a live session."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oarfish_amd import _lib
from oarfish_amd import build as _b
from oarfish_amd.em import CellsStream, UmiRuleC
from oarfish_amd.single_cell import SingleCellArgs, quantify_single_cell_from_record_batches
from tests.test_cells_umis_stream import FILTERS, T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["oem_cells_stream_set_umi_rule", "oem_cells_stream_umi_rule_copy"]
TL = np.full(T, 2000, dtype=np.uint64)
GENE_OF = [0, 0, 1, 1, 2, 2, 3, 3]


def test_declared_exported_by_both_libraries_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "oarfish_em.h")).read(), flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
        assert m, "include/oarfish_em.h does not declare " + name
        assert len(m.group(1).split(",")) == 2
        assert name in _lib.ABI_SYMBOLS and name in _b.header_symbols()
        assert len(getattr(_lib.lib(), name).argtypes) == 2
    for path in (_b.LIB_PATH, _b.TESTING_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert set(NEW) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, path
    assert re.search(r"#define OEM_CELLS_STREAM_INFO_UMI_CORRECTED_READS\s+12u", src) and _lib.OEM_CELLS_STREAM_INFO_UMI_CORRECTED_READS == 12
    assert "#define OEM_ABI_VERSION 2" in src and C.sizeof(_lib.CellsStreamOptsC) == 88 and C.sizeof(UmiRuleC) == 16
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in doc, "INTEGRATION.md does not name " + name
    # the sentences that said the sessions keep the exact rule are gone
    for path in ("include/oarfish_em.h", "README.md", "DESIGN.md", "INTEGRATION.md"):
        text = " ".join(open(os.path.join(ROOT, path)).read().split())
        assert "keep the exact rule" not in text, path


def test_null_sessions_and_sessions_without_a_device():
    L = _lib.lib()
    rule = UmiRuleC(None, 0, 0)
    assert L.oem_cells_stream_set_umi_rule(None, C.addressof(rule)) == _lib.OEM_ERR_ARG and b"NULL session" in L.oem_last_error()
    assert b"oem_cells_stream_set_umi_rule" in L.oem_last_error()
    assert L.oem_cells_stream_umi_rule_copy(None, None) == _lib.OEM_ERR_ARG and b"NULL session" in L.oem_last_error()
    assert b"oem_cells_stream_umi_rule_copy" in L.oem_last_error()
    if _lib.device_count() > 0:
        return
    for collated in (True, False):
        with pytest.raises(_lib.OemError) as ei:
            CellsStream(T, filters=FILTERS, txp_len=TL, barcodes=True, collated=collated, umis=True, gene_of=GENE_OF, umi_correct=True)
        assert ei.value.code == _lib.OEM_ERR_NO_DEVICE


def test_the_wrapper_checks_its_own_arguments():
    with pytest.raises(ValueError, match="umis=True"):
        CellsStream(T, filters=FILTERS, txp_len=TL, barcodes=True, gene_of=GENE_OF)
    with pytest.raises(ValueError, match="umis=True"):
        CellsStream(T, filters=FILTERS, txp_len=TL, barcodes=True, umi_correct=True)
    with pytest.raises(ValueError, match="umis=True"):
        CellsStream(T, umi_correct=True)
    for bad in (GENE_OF[:-1], GENE_OF + [0], [GENE_OF], 3):
        with pytest.raises(ValueError, match="n_txps entries"):
            CellsStream(T, filters=FILTERS, txp_len=TL, barcodes=True, umis=True, gene_of=bad)


def test_the_driver_checks_its_own_arguments(tmp_path):
    """Every one of these is a ValueError before any device use: no session is created, nothing is written."""
    a = SingleCellArgs(output="x")
    assert a.gene_of is None and a.gene_names is None and a.umi_correct is False and a.gene_counts is False
    names = [f"t{i}" for i in range(T)]
    genes = [f"g{i}" for i in range(4)]
    out = str(tmp_path / "sub" / "out")

    def run(**kw):
        def batches():
            raise AssertionError("the batches were read")
            yield
        return quantify_single_cell_from_record_batches(FILTERS, names, TL, batches(), SingleCellArgs(output=out, **kw))

    for kw, words in [
        (dict(gene_counts=True), "gene_of and gene_names"),
        (dict(gene_counts=True, gene_of=GENE_OF), "gene_of and gene_names"),
        (dict(gene_counts=True, gene_names=genes), "gene_of and gene_names"),
        (dict(gene_counts=True, gene_of=GENE_OF, gene_names=genes[:3]), "gene_names must name the 4 genes"),
        (dict(gene_counts=True, gene_of=GENE_OF, gene_names=genes + ["g4"]), "gene_names must name the 4 genes"),
        (dict(gene_counts=True, gene_of=GENE_OF[:-1], gene_names=genes), "one gene id per transcript"),
        (dict(umis=True, gene_of=GENE_OF + [3]), "one gene id per transcript"),
        (dict(gene_counts=True, gene_of=[-1] + GENE_OF[1:], gene_names=genes), "from 0"),
        (dict(umi_correct=True), "umi_correct goes with umis"),
        (dict(umi_correct=True, gene_counts=True, gene_of=GENE_OF, gene_names=genes), "umi_correct goes with umis"),
        (dict(gene_of=GENE_OF), "gene_of goes with umis"),
    ]:
        with pytest.raises(ValueError, match=words):
            run(**kw)
    assert not os.path.exists(os.path.dirname(out))
