"""CPU tests of the sparse per-cell results (oem_em_run_cells_sparse): argument checks before any device use, the
result handle's NULL contract, and the host side of the CSR form -- `writers.csr_triplets` gives exactly the triplets
`writers.cell_triplets` takes from the dense matrix, so `.count.mtx` is the same file either way."""
import ctypes as C

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib
from oarfish_amd import writers as W


def dense_to_csr(x):
    """single_cell.rs:151-160 on a dense cells x transcripts f64 matrix: per row the v > 0 entries in ascending
    column, as f32 -- the form em_cells_sparse returns."""
    x = np.asarray(x, dtype=np.float64)
    keep = x > 0.0
    indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.uint64)
    rows, cols = np.nonzero(keep)
    return indptr, cols.astype(np.uint32), x[rows, cols].astype(np.float32)


def _cells():
    """Two cells of two reads each over three transcripts."""
    cell_off = np.array([0, 2, 4], dtype=np.uint64)
    rp = np.array([0, 1, 3, 4, 6], dtype=np.uint64)
    tid = np.array([0, 1, 2, 2, 0, 1], dtype=np.uint32)
    p = np.ones(6, dtype=np.float32)
    return cell_off, rp, tid, p


def _call(cell_off, rp, tid, p, n_txps=3, out=True):
    L = _lib.lib()
    res = C.c_void_p(12345)   # must come back NULL on failure
    rc = L.oem_em_run_cells_sparse(cell_off.ctypes.data, len(cell_off) - 1, rp.ctypes.data, tid.ctypes.data,
                                   p.ctypes.data, None, len(rp) - 1, len(tid), n_txps, 0, 100, 1e-3,
                                   C.byref(res) if out else None)
    return rc, res


def test_sparse_entry_points_are_exported():
    L = _lib.lib()
    for name in ("oem_em_run_cells_sparse", "oem_cells_result_dims", "oem_cells_result_copy", "oem_cells_result_destroy"):
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS
    assert callable(oarfish_amd.em_cells_sparse) and "em_cells_sparse" in oarfish_amd.__all__


def test_sparse_argument_validation_precedes_device_use():
    cell_off, rp, tid, p = _cells()
    rc, _ = _call(cell_off, rp, tid, p, out=False)
    assert rc == _lib.OEM_ERR_ARG
    rc, res = _call(np.array([1, 2, 4], dtype=np.uint64), rp, tid, p)           # cell_row_off[0] != 0
    assert rc == _lib.OEM_ERR_ARG and res.value is None
    assert b"cell_row_off" in _lib.lib().oem_last_error()
    rc, res = _call(np.array([0, 3, 2, 4], dtype=np.uint64), rp, tid, p)        # decreasing offsets
    assert rc == _lib.OEM_ERR_ARG and res.value is None
    assert b"non-decreasing" in _lib.lib().oem_last_error()
    bad = tid.copy()
    bad[3] = 3                                                                  # tid >= n_txps
    rc, res = _call(cell_off, rp, bad, p)
    assert rc == _lib.OEM_ERR_ARG and res.value is None
    assert b"n_txps" in _lib.lib().oem_last_error()
    rc, res = _call(cell_off, rp, tid, p, n_txps=0)
    assert rc == _lib.OEM_ERR_ARG and res.value is None


def test_sparse_fails_loudly_without_a_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    cell_off, rp, tid, p = _cells()
    rc, res = _call(cell_off, rp, tid, p)
    assert rc == _lib.OEM_ERR_NO_DEVICE and res.value is None
    with pytest.raises(oarfish_amd.OemError) as ei:
        oarfish_amd.em_cells_sparse(cell_off, rp, tid, p, None, 3)
    assert ei.value.code == _lib.OEM_ERR_NO_DEVICE


def test_result_handle_null_contract():
    L = _lib.lib()
    n, e = C.c_uint32(7), C.c_uint64(7)
    assert L.oem_cells_result_dims(None, C.byref(n), C.byref(e)) == _lib.OEM_ERR_ARG
    assert L.oem_cells_result_copy(None, None, None, None, None) == _lib.OEM_ERR_ARG
    L.oem_cells_result_destroy(None)   # no-op


def _random_counts(rng, n_cells, T):
    x = rng.lognormal(0.0, 3.0, size=(n_cells, T))
    x[rng.random((n_cells, T)) < 0.6] = 0.0
    tiny = rng.random((n_cells, T)) < 0.05                 # f32 denormals and values that round to 0 in f32
    x[tiny] = rng.choice([1e-40, 3e-45, 1e-46, 1e-310, 5e-324], size=int(tiny.sum()))
    x[rng.random((n_cells, T)) < 0.01] = -0.0
    x[3] = 0.0                                              # a cell without entries
    return x


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_csr_triplets_equal_cell_triplets(seed):
    rng = np.random.default_rng(seed)
    x = _random_counts(rng, 9, 257)
    r0, c0, v0 = W.cell_triplets(x)
    r1, c1, v1 = W.csr_triplets(*dense_to_csr(x))
    for a, b in ((r0, r1), (c0, c1)):
        assert a.dtype == b.dtype == np.uint32
        np.testing.assert_array_equal(a, b)
    assert v0.dtype == v1.dtype == np.float32
    assert v0.tobytes() == v1.tobytes()
    # every row empty, and no rows at all
    z = np.zeros((4, 10))
    assert all(len(a) == 0 for a in W.csr_triplets(*dense_to_csr(z)))
    rows, cols, vals = W.csr_triplets(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32))
    assert len(rows) == len(cols) == len(vals) == 0


def test_count_mtx_from_either_form_is_byte_identical(tmp_path):
    rng = np.random.default_rng(11)
    x = _random_counts(rng, 6, 40)
    names = [f"t{i}" for i in range(x.shape[1])]
    barcodes = [f"BC{i}" for i in range(x.shape[0])]
    W.write_single_cell_output(str(tmp_path / "dense"), {"k": 1}, names, barcodes, x.shape[0], *W.cell_triplets(x))
    W.write_single_cell_output(str(tmp_path / "sparse"), {"k": 1}, names, barcodes, x.shape[0],
                               *W.csr_triplets(*dense_to_csr(x)))
    for ext in (".count.mtx", ".features.txt", ".barcodes.txt", ".meta_info.json"):
        assert (tmp_path / ("dense" + ext)).read_bytes() == (tmp_path / ("sparse" + ext)).read_bytes(), ext
