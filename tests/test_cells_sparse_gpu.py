"""GPU tests of the sparse per-cell results (oem_em_run_cells_sparse / em_cells_sparse): the CSR the device picks out
is what single_cell.rs:151-160 keeps (v > 0 as f32, ascending column) -- against the per-cell oracle, against the
dense call on every path of the per-cell driver, at the size of one GPU's slice of BASELINE configs[4], and on an
annotation whose dense result the caller could hardly hold."""
import os

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth
from oarfish_amd import writers as W
from oracle import c_oracle
from tests.common import assert_cell_matches_oracle, assert_counts_close

pytestmark = pytest.mark.gpu

RTOL = 1e-4  # north_star tolerance
THREADS = min(16, os.cpu_count() or 4)


def _check_structure(indptr, cols, vals, n_cells, T):
    assert indptr.dtype == np.uint64 and cols.dtype == np.uint32 and vals.dtype == np.float32
    assert len(indptr) == n_cells + 1 and int(indptr[0]) == 0 and int(indptr[-1]) == len(cols) == len(vals)
    assert np.all(np.diff(indptr.astype(np.int64)) >= 0)
    assert np.all(vals > 0) and np.all(np.isfinite(vals)) and (len(cols) == 0 or int(cols.max()) < T)
    rows = np.repeat(np.arange(n_cells), np.diff(indptr.astype(np.int64)))
    same_row = rows[1:] == rows[:-1]
    assert np.all(np.diff(cols.astype(np.int64))[same_row] > 0), "columns not strictly ascending inside a row"


def _row(indptr, cols, vals, c, T):
    out = np.zeros(T)
    s = slice(int(indptr[c]), int(indptr[c + 1]))
    out[cols[s]] = vals[s]
    return out


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def assert_sparse_equals_dense(sp, dense, dense_infos, cell_off, label):
    """Sparse = cell_triplets(dense): identical columns, values within one f32 ulp (two runs differ in the last f64
    bits: atomics); a cell whose run stopped one iteration apart is held to the north star instead."""
    indptr, cols, vals, infos = sp
    n_cells, T = dense.shape
    _check_structure(indptr, cols, vals, n_cells, T)
    assert len(infos) == len(dense_infos) == n_cells
    rs, cs, vs = W.csr_triplets(indptr, cols, vals)
    rd, cd, vd = W.cell_triplets(dense)
    agree = np.array([infos[c].niter == dense_infos[c].niter for c in range(n_cells)], dtype=bool)
    if agree.all():
        np.testing.assert_array_equal(rs, rd, err_msg=label)
        np.testing.assert_array_equal(cs, cd, err_msg=label)
        assert _ulps(vs, vd).max(initial=0) <= 1, f"{label}: values differ by more than one f32 ulp"
        return
    for c in range(n_cells):
        assert abs(infos[c].niter - dense_infos[c].niter) <= 1, (label, c, infos[c], dense_infos[c])
        s = slice(int(indptr[c]), int(indptr[c + 1]))
        want = np.nonzero(dense[c] > 0.0)[0]
        if agree[c]:
            np.testing.assert_array_equal(cols[s], want, err_msg=f"{label}: cell {c}")
            assert _ulps(vals[s], dense[c][want].astype(np.float32)).max(initial=0) <= 1, f"{label}: cell {c}"
        else:
            assert_counts_close(_row(indptr, cols, vals, c, T), dense[c], int(cell_off[c + 1] - cell_off[c]), T, RTOL,
                                f"{label}: cell {c}")


def _cell_store(cell_off, row_ptr, tid, p, cov, c, T):
    r0, r1 = int(cell_off[c]), int(cell_off[c + 1])
    a0, a1 = int(row_ptr[r0]), int(row_ptr[r1])
    return (c_oracle.Store(row_ptr[r0:r1 + 1] - row_ptr[r0], tid[a0:a1], p[a0:a1], None if cov is None else cov[a0:a1], T),
            r1 - r0)


def _against_oracle(sp, cell_off, row_ptr, tid, p, cov, T, cells, max_iter, label):
    indptr, cols, vals, infos = sp
    for c in cells:
        o, n = _cell_store(cell_off, row_ptr, tid, p, cov, c, T)
        want, wi = c_oracle.do_em(o, max_iter=max_iter, conv_thresh=1e-3, min_iter_gate=50)
        assert abs(infos[c].niter - wi.niter) <= 1, (label, c, infos[c], wi.niter)
        got = _row(indptr, cols, vals, c, T)
        if infos[c].niter == wi.niter:
            s = slice(int(indptr[c]), int(indptr[c + 1]))
            np.testing.assert_array_equal(cols[s], np.nonzero(want > 0.0)[0], err_msg=f"{label}: cell {c}")
        assert_counts_close(got, want, n, T, RTOL, f"{label}: cell {c}")


@pytest.mark.parametrize("with_nan", [False, True])
def test_sparse_cells_match_per_cell_oracle(with_nan):
    """single_cell.rs:139-160 per cell, the kept entries of :151-160, against the oracle's em::em (gate 50); with a
    coverage column whose NaN rows drop their reads (em.rs:115)."""
    n_cells, T = 6, 500
    cell_off, row_ptr, tid, p = synth.make_cells(n_cells, 3_000, T, seed=9)
    cov = None
    if with_nan:
        rng = np.random.default_rng(5)
        cov = rng.uniform(0.05, 1.0, len(tid))
        for r in rng.choice(len(row_ptr) - 1, 40, replace=False):
            a0, a1 = int(row_ptr[r]), int(row_ptr[r + 1])
            cov[a0 + int(rng.integers(0, a1 - a0))] = np.nan
    sp = oarfish_amd.em_cells_sparse(cell_off, row_ptr, tid, p, cov, T, max_iter=300, convergence_thresh=1e-3)
    _check_structure(*sp[:3], n_cells, T)
    _against_oracle(sp, cell_off, row_ptr, tid, p, cov, T, range(n_cells), 300, f"nan={with_nan}")


def _with_empty_cells(cell_off):
    """Cells without reads before, between and after the generated ones."""
    o = [int(x) for x in cell_off]
    return np.array([0, 0] + o[1:2] + o[1:3] + [o[3], o[3]] + o[4:] + [o[-1]], dtype=np.uint64)


PATHS = ["batched", "serial", "groups", "uncompacted", "max_iter_0", "one_cell", "no_cells", "empty_cells"]


@pytest.mark.parametrize("path", PATHS)
def test_sparse_equals_dense_on_every_path(path, monkeypatch):
    n_cells, T = 10, 900
    cell_off, row_ptr, tid, p = synth.make_cells(n_cells, 3_000, T, seed=31, expressed_frac=0.2)
    max_iter = 200
    knobs = {}
    if path == "serial":
        knobs["OEM_SERIAL_CELLS"] = "1"
    elif path == "groups":   # pairs of cells per group: at least five groups for the two workers
        nnz = np.diff(row_ptr[cell_off.astype(np.int64)].astype(np.int64))
        limit = int((nnz[1:] + nnz[:-1]).max())
        groups, c0 = 0, 0
        while c0 < n_cells:
            c1 = c0 + 1
            while c1 < n_cells and nnz[c0:c1 + 1].sum() <= limit:
                c1 += 1
            groups, c0 = groups + 1, c1
        assert groups >= 5
        knobs["OEM_CELLS_GROUP_NNZ"] = str(limit)
    elif path == "uncompacted":
        knobs["OEM_TEST_FAIL_RANK_ALLOC"] = "1"
    elif path == "max_iter_0":
        max_iter = 0
    elif path == "one_cell":
        r1 = int(cell_off[1])
        cell_off, row_ptr = cell_off[:2], row_ptr[:r1 + 1]
        tid, p = tid[:int(row_ptr[-1])], p[:int(row_ptr[-1])]
    elif path == "no_cells":
        cell_off, row_ptr, tid, p = (np.zeros(1, np.uint64), np.zeros(1, np.uint64), np.zeros(0, np.uint32),
                                     np.zeros(0, np.float32))
    elif path == "empty_cells":
        cell_off = _with_empty_cells(cell_off)
    n = len(cell_off) - 1
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    args = (cell_off, row_ptr, tid, p, None, T)
    if knobs:   # the knobs exist only in the test-only library
        with _lib.testing():
            sp = oarfish_amd.em_cells_sparse(*args, max_iter=max_iter, convergence_thresh=1e-3)
            dense, dinfos = oarfish_amd.em_cells(*args, max_iter=max_iter, convergence_thresh=1e-3)
    else:
        sp = oarfish_amd.em_cells_sparse(*args, max_iter=max_iter, convergence_thresh=1e-3)
        dense, dinfos = oarfish_amd.em_cells(*args, max_iter=max_iter, convergence_thresh=1e-3)
    assert_sparse_equals_dense(sp, dense, dinfos, cell_off, path)
    indptr = sp[0]
    counts = np.diff(indptr.astype(np.int64))
    reads = np.diff(cell_off.astype(np.int64))
    assert np.all(counts[reads == 0] == 0)
    for c in np.nonzero(reads)[0]:   # mass conservation per cell (f32 values)
        s = slice(int(indptr[c]), int(indptr[c + 1]))
        assert abs(sp[2][s].astype(np.float64).sum() - reads[c]) < 1e-6 * reads[c], (path, c)
    if path in ("batched", "serial", "max_iter_0"):
        _against_oracle(sp, cell_off, row_ptr, tid, p, None, T, (0, n - 1), max_iter, path)


@pytest.mark.timeout(900)
def test_sparse_c5_slice_of_one_gpu():
    """The 625 x 50 k-read slice of BASELINE configs[4] over 60 k transcripts (the 1 : 3 head split, compacted batched
    groups on two workers): sparse = dense, per-cell mass, unique <= val <= total, four cells of the tail group against
    the oracle, and the result at most half the bytes of the dense one."""
    n_cells, per_cell, T = 625, 50_000, 60_000
    cell_off, row_ptr, tid, p = synth.make_cells(n_cells, per_cell, T, seed=37, threads=THREADS)
    sp = oarfish_amd.em_cells_sparse(cell_off, row_ptr, tid, p, None, T, max_iter=1000, convergence_thresh=1e-3)
    dense, dinfos = oarfish_amd.em_cells(cell_off, row_ptr, tid, p, None, T, max_iter=1000, convergence_thresh=1e-3)
    assert_sparse_equals_dense(sp, dense, dinfos, cell_off, "625-cell slice")
    del dense
    indptr, cols, vals, infos = sp
    sums = np.add.reduceat(vals.astype(np.float64), indptr[:-1].astype(np.int64))
    assert np.abs(sums - per_cell).max() < 1e-6 * per_cell
    for c in (0, 311, 624):   # unique <= val <= total, from the cell's own alignments (f32 rounding allowed)
        r0, r1 = int(cell_off[c]), int(cell_off[c + 1])
        a0, a1 = int(row_ptr[r0]), int(row_ptr[r1])
        lens = (row_ptr[r0 + 1:r1 + 1] - row_ptr[r0:r1]).astype(np.int64)
        tot = np.bincount(tid[a0:a1], minlength=T)
        uniq = np.bincount(tid[a0:a1][np.repeat(lens == 1, lens)], minlength=T)
        got = _row(indptr, cols, vals, c, T)
        eps = 2.0 ** -23
        assert np.all(got >= uniq * (1 - eps) - 1e-6) and np.all(got <= tot * (1 + eps) + 1e-6), c
    for c in (156, 157, 400, 624):   # cells of the tail group (625 // 4 = 156 head cells) against the oracle
        o, n = _cell_store(cell_off, row_ptr, tid, p, None, c, T)
        want = c_oracle.do_em(o, max_iter=1000, conv_thresh=1e-3, min_iter_gate=50)
        s = slice(int(indptr[c]), int(indptr[c + 1]))
        assert_cell_matches_oracle(infos[c], want, n, T, f"cell {c}", cols=cols[s], vals=vals[s])
    dense_bytes = n_cells * T * 8
    frac = len(cols) * 8 / dense_bytes
    print(f"625-cell slice: {len(cols)} entries, {frac:.3f} of the dense result's bytes")
    assert frac <= 0.5, frac


@pytest.mark.timeout(900)
def test_sparse_cells_on_a_human_sized_annotation():
    """1 000 cells x 20 k reads over 250 k transcripts, each cell expressing 5 % of them: the dense result would be
    2 GB of host memory; the sparse one holds only the non-zeros."""
    n_cells, per_cell, T = 1_000, 20_000, 250_000
    cell_off, row_ptr, tid, p = synth.make_cells(n_cells, per_cell, T, seed=41, expressed_frac=0.05, threads=THREADS)
    sp = oarfish_amd.em_cells_sparse(cell_off, row_ptr, tid, p, None, T, max_iter=1000, convergence_thresh=1e-3)
    indptr, cols, vals, infos = sp
    _check_structure(indptr, cols, vals, n_cells, T)
    sums = np.add.reduceat(vals.astype(np.float64), indptr[:-1].astype(np.int64))
    assert np.abs(sums - per_cell).max() < 1e-6 * per_cell
    counts = np.diff(indptr.astype(np.int64))
    for c in range(n_cells):
        a0, a1 = int(row_ptr[int(cell_off[c])]), int(row_ptr[int(cell_off[c + 1])])
        assert counts[c] <= len(np.unique(tid[a0:a1])), c
    _against_oracle(sp, cell_off, row_ptr, tid, p, None, T, (0, 1, 499, 998, 999), 1000, "250 k annotation")
    result_bytes = 8 * (n_cells + 1) + 8 * len(cols)
    print(f"250 k annotation: {len(cols)} entries, {result_bytes / 1e6:.1f} MB against {n_cells * T * 8 / 1e9:.1f} GB dense")
    assert result_bytes < n_cells * T * 8 / 10
