"""GPU tests of the fused per-cell coverage model + EM (oem_em_run_cells_coverage_sparse / em_cells_coverage_sparse):
its result is cells_coverage_probs followed by em_cells_sparse on that column -- against the oracle cell by cell,
against that composition on every path of the per-cell driver and with the coverage forced into sub-chunks, through
the column it returns, on errors, and at the size of one GPU's slice of BASELINE configs[4]."""
import contextlib
import os

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth
from oracle import c_oracle
from oracle import filter_py as fp
from tests.common import assert_cell_matches_oracle, assert_counts_close
from tests.test_cells_coverage_gpu import _per_cell_loop

pytestmark = pytest.mark.gpu

RTOL = 1e-4  # north_star tolerance
THREADS = min(16, os.cpu_count() or 4)


# ---- comparison helpers (as in test_cells_sparse_gpu.py) ---------------------------------------------------------
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


def assert_sparse_equal(got, want, cell_off, T, label, cells=None):
    """Two sparse results of the same problem: where a cell's iteration counts agree, identical columns and values
    within one f32 ulp (two runs differ in the last f64 bits: atomics); a cell whose run stopped one iteration apart
    is held to the north star instead."""
    gi, gc, gv, ginf = got
    wi, wc, wv, winf = want
    n_cells = len(cell_off) - 1
    _check_structure(gi, gc, gv, n_cells, T)
    assert len(ginf) == len(winf) == n_cells
    for c in range(n_cells) if cells is None else cells:
        assert abs(ginf[c].niter - winf[c].niter) <= 1, (label, c, ginf[c], winf[c])
        gs, ws = slice(int(gi[c]), int(gi[c + 1])), slice(int(wi[c]), int(wi[c + 1]))
        if ginf[c].niter == winf[c].niter:
            np.testing.assert_array_equal(gc[gs], wc[ws], err_msg=f"{label}: cell {c}")
            assert _ulps(gv[gs], wv[ws]).max(initial=0) <= 1, f"{label}: cell {c}: values differ by more than one f32 ulp"
        else:
            assert_counts_close(_row(gi, gc, gv, c, T), _row(wi, wc, wv, c, T).astype(np.float64),
                                int(cell_off[c + 1] - cell_off[c]), T, RTOL, f"{label}: cell {c}")


def _slices(cell_off, row_ptr, c):
    r0, r1 = int(cell_off[c]), int(cell_off[c + 1])
    return r0, r1, int(row_ptr[r0]), int(row_ptr[r1])


def _oracle_cov(cell_off, row_ptr, tid, s, e, tl, bin_width, model, growth):
    want = np.zeros(len(tid))
    for c in range(len(cell_off) - 1):
        r0, r1, a0, a1 = _slices(cell_off, row_ptr, c)
        st = fp.Store(row_ptr=[int(x) - a0 for x in row_ptr[r0:r1 + 1]], tid=[int(x) for x in tid[a0:a1]],
                      start=[int(x) for x in s[a0:a1]], end=[int(x) for x in e[a0:a1]])
        want[a0:a1] = fp.coverage_probs(st, [int(x) for x in tl], bin_width, growth, model=model)
    return want


def _composition(cell_off, row_ptr, tid, p, s, e, tl, max_iter=1000, **kw):
    cov = oarfish_amd.cells_coverage_probs(cell_off, row_ptr, tid, s, e, tl, **kw)
    return oarfish_amd.em_cells_sparse(cell_off, row_ptr, tid, p, cov, len(tl), max_iter=max_iter,
                                       convergence_thresh=1e-3), cov


# ---- against the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,growth", [("binomial", 2.0), ("logistic", 0.8)])
def test_fused_matches_the_oracle_cell_by_cell(model, growth):
    """filter_py.coverage_probs + the oracle's em::em per cell (gate 50, 1000 iterations, 1e-3): the same kept
    columns where the iteration counts agree, counts within the north star.  Zero-span alignments drop their reads
    on both sides (em.rs:115)."""
    n_cells, T = 6, 200
    cell_off, row_ptr, tid, p = synth.make_cells(n_cells, 800, T, kbar=5.0, seed=83)
    tl, s, e = synth.make_coordinates(tid, T, seed=83, zero_span_frac=0.005)
    indptr, cols, vals, infos = oarfish_amd.em_cells_coverage_sparse(cell_off, row_ptr, tid, p, s, e, tl, model=model,
                                                                     growth_rate=growth)
    _check_structure(indptr, cols, vals, n_cells, T)
    want_cov = _oracle_cov(cell_off, row_ptr, tid, s, e, tl, 100, model, growth)
    assert np.isnan(want_cov).sum() > 0
    for c in range(n_cells):
        r0, r1, a0, a1 = _slices(cell_off, row_ptr, c)
        o = c_oracle.Store(row_ptr[r0:r1 + 1] - row_ptr[r0], tid[a0:a1], p[a0:a1], want_cov[a0:a1], T)
        want, wi = c_oracle.do_em(o, max_iter=1000, conv_thresh=1e-3, min_iter_gate=50)
        assert abs(infos[c].niter - wi.niter) <= 1, (c, infos[c], wi.niter)
        sl = slice(int(indptr[c]), int(indptr[c + 1]))
        if infos[c].niter == wi.niter:
            np.testing.assert_array_equal(cols[sl], np.nonzero(want > 0.0)[0], err_msg=f"cell {c}")
        assert_counts_close(_row(indptr, cols, vals, c, T), want, r1 - r0, T, RTOL, f"{model}: cell {c}")


# ---- against the composition, on every path of the driver ----------------------------------------------------------
def _with_empty_cells(cell_off):
    o = [int(x) for x in cell_off]
    return np.array([0, 0] + o[1:2] + o[1:3] + [o[3], o[3]] + o[4:] + [o[-1]], dtype=np.uint64)


PATHS = ["batched", "serial", "groups", "uncompacted", "max_iter_0", "one_cell", "no_cells", "empty_cells",
         "cov_sub_chunks", "host_layout"]


@pytest.mark.parametrize("path", PATHS)
def test_fused_equals_the_composition_on_every_path(path, monkeypatch):
    n_cells, T = 10, 900
    cell_off, row_ptr, tid, p = synth.make_cells(n_cells, 3_000, T, seed=31, expressed_frac=0.2)
    tl, s, e = synth.make_coordinates(tid, T, seed=31, zero_span_frac=0.002)
    max_iter = 200
    knobs = {}
    if path == "serial":
        knobs["OEM_SERIAL_CELLS"] = "1"
    elif path == "groups":   # pairs of cells per group: several groups for the two workers
        nnz = np.diff(row_ptr[cell_off.astype(np.int64)].astype(np.int64))
        knobs["OEM_CELLS_GROUP_NNZ"] = str(int((nnz[1:] + nnz[:-1]).max()))
    elif path == "uncompacted":
        knobs["OEM_TEST_FAIL_RANK_ALLOC"] = "1"
    elif path == "max_iter_0":
        max_iter = 0
    elif path == "one_cell":
        r1 = int(cell_off[1])
        cell_off, row_ptr = cell_off[:2], row_ptr[:r1 + 1]
        a1 = int(row_ptr[-1])
        tid, p, s, e = tid[:a1], p[:a1], s[:a1], e[:a1]
    elif path == "no_cells":
        cell_off, row_ptr = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
        tid, p, s, e = np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    elif path == "empty_cells":
        cell_off = _with_empty_cells(cell_off)
    elif path == "cov_sub_chunks":   # a bin budget of about two cells: the group's coverage runs in sub-chunks
        knobs["OEM_COV_CELLS_CHUNK_BINS"] = "60000"
    elif path == "host_layout":      # the host layout builder takes the batched store: the weights come back
        knobs["OEM_TEST_HOST_LAYOUT"] = "1"
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    with _lib.testing() if knobs else contextlib.nullcontext():   # (knobs: the test-only library)
        fused = oarfish_amd.em_cells_coverage_sparse(cell_off, row_ptr, tid, p, s, e, tl, max_iter=max_iter)
        comp, cov = _composition(cell_off, row_ptr, tid, p, s, e, tl, max_iter=max_iter)
    n = len(cell_off) - 1
    assert_sparse_equal(fused, comp, cell_off, T, path)
    indptr, cols, vals, infos = fused
    reads = np.diff(cell_off.astype(np.int64))
    counts = np.diff(indptr.astype(np.int64))
    assert np.all(counts[reads == 0] == 0)
    if path not in ("no_cells",):
        # a cell's mass is its reads less the ones the NaN coverage of a zero-span alignment drops
        nan_read = np.zeros(len(row_ptr) - 1, bool)
        bad = np.nonzero(np.isnan(cov))[0]
        nan_read[np.searchsorted(row_ptr.astype(np.int64), bad, side="right") - 1] = True
        for c in np.nonzero(reads)[0]:
            live = reads[c] - int(nan_read[int(cell_off[c]):int(cell_off[c + 1])].sum())
            got = vals[int(indptr[c]):int(indptr[c + 1])].astype(np.float64).sum()
            assert abs(got - live) < 1e-5 * max(live, 1), (path, c, got, live)
    assert len(infos) == n


# ---- the column the EM used ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["binomial", "logistic"])
def test_returned_column_gives_the_fused_result(model):
    """em_cells_sparse on the column the fused call returns is the fused result; the column is cells_coverage_probs'
    to 1e-12, with NaN in the same places."""
    n_cells, T = 12, 1_500
    cell_off, row_ptr, tid, p = synth.make_cells(n_cells, 4_000, T, seed=47, expressed_frac=0.3)
    tl, s, e = synth.make_coordinates(tid, T, seed=47, zero_span_frac=0.003)
    *fused, cov = oarfish_amd.em_cells_coverage_sparse(cell_off, row_ptr, tid, p, s, e, tl, model=model,
                                                       return_coverage=True)
    want_cov = oarfish_amd.cells_coverage_probs(cell_off, row_ptr, tid, s, e, tl, model=model)
    assert np.isnan(want_cov).sum() > 0
    assert np.array_equal(np.isnan(cov), np.isnan(want_cov))
    fin = ~np.isnan(want_cov)
    np.testing.assert_allclose(cov[fin], want_cov[fin], rtol=1e-12, atol=0)
    again = oarfish_amd.em_cells_sparse(cell_off, row_ptr, tid, p, cov, T)
    assert_sparse_equal(tuple(fused), again, cell_off, T, f"EM half ({model})")


# ---- errors --------------------------------------------------------------------------------------------------------
def test_an_alignment_past_its_transcript_names_the_cell():
    n_cells, T = 8, 300
    cell_off, row_ptr, tid, p = synth.make_cells(n_cells, 500, T, seed=89)
    tl, s, e = synth.make_coordinates(tid, T, seed=89, zero_span_frac=0.01)
    bad_cell = 5
    _, _, a0, a1 = _slices(cell_off, row_ptr, bad_cell)
    e_bad = e.copy()
    j = a0 + (a1 - a0) // 2
    e_bad[j] = np.uint32(int(tl[tid[j]]) + 500)
    with pytest.raises(oarfish_amd.OemError) as ei:
        oarfish_amd.em_cells_coverage_sparse(cell_off, row_ptr, tid, p, s, e_bad, tl)
    assert ei.value.code == _lib.OEM_ERR_STATE
    assert f"cell {bad_cell}:" in str(ei.value) and "outside its transcript" in str(ei.value)
    fused = oarfish_amd.em_cells_coverage_sparse(cell_off, row_ptr, tid, p, s, e, tl)
    comp, _ = _composition(cell_off, row_ptr, tid, p, s, e, tl)
    assert_sparse_equal(fused, comp, cell_off, T, "after an error")


# ---- one GPU's slice of BASELINE configs[4] ------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_fused_c5_slice_of_one_gpu():
    """625 cells x 50 k reads over 60 k transcripts in one call (the 1 : 3 head split, two workers): per-cell mass,
    16 sampled cells against the composition, and four cells of the tail group against the oracle's em::em on the
    per-cell device coverage."""
    n_cells, per_cell, T = 625, 50_000, 60_000
    cell_off, row_ptr, tid, p = synth.make_cells(n_cells, per_cell, T, seed=37, threads=THREADS)
    tl, s, e = synth.make_coordinates(tid, T, seed=37, zero_span_frac=0.001, threads=THREADS)
    fused = oarfish_amd.em_cells_coverage_sparse(cell_off, row_ptr, tid, p, s, e, tl)
    indptr, cols, vals, infos = fused
    _check_structure(indptr, cols, vals, n_cells, T)
    sums = np.add.reduceat(vals.astype(np.float64), indptr[:-1].astype(np.int64))
    assert np.all(sums <= per_cell * (1 + 1e-6)) and np.all(sums > per_cell * 0.98), (sums.min(), sums.max())
    comp, cov = _composition(cell_off, row_ptr, tid, p, s, e, tl)
    cells = np.random.default_rng(3).choice(n_cells, 16, replace=False)
    assert_sparse_equal(fused, comp, cell_off, T, "625-cell slice", cells=cells)
    # exact mass: a cell's reads less the ones a NaN coverage drops
    nan_rows = np.unique(np.searchsorted(row_ptr.astype(np.int64), np.nonzero(np.isnan(cov))[0], side="right") - 1)
    dropped = np.bincount(np.searchsorted(cell_off.astype(np.int64), nan_rows, side="right") - 1, minlength=n_cells)
    np.testing.assert_allclose(sums, per_cell - dropped, rtol=1e-6)
    # cells of the tail group (625 // 4 = 156 head cells) against the oracle's EM on the per-cell device coverage
    tail = (156, 157, 400, 624)
    col = _per_cell_loop(cell_off, row_ptr, tid, s, e, tl, 100, 1, 2.0, cells=tail)
    for c in tail:
        r0, r1, a0, a1 = _slices(cell_off, row_ptr, c)
        o = c_oracle.Store(row_ptr[r0:r1 + 1] - row_ptr[r0], tid[a0:a1], p[a0:a1], col[a0:a1], T)
        want = c_oracle.do_em(o, max_iter=1000, conv_thresh=1e-3, min_iter_gate=50)
        sl = slice(int(indptr[c]), int(indptr[c + 1]))
        assert_cell_matches_oracle(infos[c], want, r1 - r0, T, f"cell {c}", cols=cols[sl], vals=vals[sl])
