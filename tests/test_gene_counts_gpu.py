"""GPU tests of oem_cells_gene_counts: the device against the host walk of oem_gene_counts.h (the testing library's hook)
and against the walk of tests/test_gene_counts.py, exactly -- cell_off and genes equal, values bit for bit.  The cases are
that file's, plus the wavefront, workgroup and scan edges (1 to 257 runs in one cell, one run per cell), one input of
65 537 entries, and a random input under OEM_GENE_BATCH_ENTRIES: 1 (every cell a batch, each larger than the bound), 300
(a batch boundary between two cells that end and start in one gene) and 299 (every cell larger than the bound)."""
import numpy as np
import pytest

from oarfish_amd import _lib, writers
from oarfish_amd.em import cells_gene_counts, count_matrix_text

from .test_gene_counts import HOOK, all_cases, call, make_case, random_case, same, walk

pytestmark = pytest.mark.gpu


def device(case, **kw):
    return cells_gene_counts(case["indptr"], case["cols"], case["vals"], case["gene_of"], n_genes=case["n_genes"], **kw)


def expected(case):
    """The walk of the test file; the host walk must agree with it first."""
    want = walk(case["indptr"], case["cols"], case["vals"], case["gene_of"])
    rc, msg, host = call(_lib.testing_lib(), HOOK, case)
    assert rc == _lib.OEM_OK and same(host, want), msg
    return want


@pytest.mark.parametrize("case", all_cases(), ids=lambda c: c["label"])
def test_device_equals_the_walks(case):
    assert same(device(case), expected(case)), case["label"]


def test_n_genes_none_is_max_plus_one():
    case = random_case()
    assert same(cells_gene_counts(case["indptr"], case["cols"], case["vals"], case["gene_of"]), expected(case))


def big_case():
    """65 537 entries in 5 cells (the middle one empty), ascending columns as the project's CSRs have them."""
    rng = np.random.default_rng(11)
    n_txps, n_genes = 30_000, 4_000
    gene_of = rng.integers(0, n_genes, size=n_txps)
    sizes = [20_000, 1, 0, 25_536, 20_000]
    assert sum(sizes) == 65_537
    cells = []
    for s in sizes:
        cols = np.sort(rng.choice(n_txps, size=s, replace=False))
        cells.append(list(zip(cols.tolist(), rng.random(s).astype(np.float32).tolist())))
    return make_case("65 537 entries", cells, gene_of, n_genes=n_genes)


def test_an_input_of_65537_entries():
    case = big_case()
    assert same(device(case), expected(case))


@pytest.fixture(scope="module")
def boundary_case():
    """8 cells x 300 entries over 40 transcripts in 12 genes; every cell ends and the next starts in one gene."""
    case = random_case()
    g = case["gene_of"]
    cols = case["cols"].reshape(8, 300).copy()
    for c in range(7):
        cols[c + 1, 0] = np.flatnonzero(g == g[cols[c, -1]])[0]
    case = dict(case, cols=cols.reshape(-1))
    for c in range(7):
        assert g[case["cols"][300 * c + 299]] == g[case["cols"][300 * (c + 1)]]
    return case, walk(case["indptr"], case["cols"], case["vals"], case["gene_of"])


@pytest.mark.parametrize("batch", [1, 299, 300, 301, 2400])
def test_batches_of_cells(monkeypatch, boundary_case, batch):
    """The product's bound is 2^27 entries; the testing library reads it from the environment."""
    case, want = boundary_case
    monkeypatch.setenv("OEM_GENE_BATCH_ENTRIES", str(batch))
    with _lib.testing():
        got = device(case)
    assert same(got, want), batch
    assert same(device(case), want)


def test_the_result_formats_as_a_count_matrix(tmp_path):
    """count_matrix_text on the result against writers.write_single_cell_output on its triplets, byte for byte; then the
    two files of write_single_cell_gene_output_device."""
    case = random_case()
    want = expected(case)
    indptr_g, genes, vals_g = device(case)
    assert same((indptr_g, genes, vals_g), want)
    names = [f"gene{g}" for g in range(case["n_genes"])]
    n_cells = len(indptr_g) - 1
    ref = str(tmp_path / "ref")
    writers.write_single_cell_output(ref, {}, names, None, n_cells, *writers.csr_triplets(*want))
    mtx = open(ref + ".count.mtx", "rb").read()
    prefix = mtx[:[i for i, b in enumerate(mtx) if b == 10][2] + 1]
    assert count_matrix_text(indptr_g, genes, vals_g, case["n_genes"], prefix=prefix).text.tobytes() == mtx
    out = str(tmp_path / "sub" / "out")
    writers.write_single_cell_gene_output_device(out, names, n_cells, indptr_g, genes, vals_g)
    assert open(out + ".gene_count.mtx", "rb").read() == mtx
    assert open(out + ".gene_features.txt").read() == "".join(n + "\n" for n in names)
    with pytest.raises(ValueError):
        writers.write_single_cell_gene_output_device(out, names, n_cells + 1, indptr_g, genes, vals_g)
