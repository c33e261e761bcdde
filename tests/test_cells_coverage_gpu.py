"""GPU tests of the per-cell coverage model (oem_coverage_probs_cells_device / cells_coverage_probs): every cell gets
its own bins, as single_cell.rs:117-137 does -- against the oracle on each cell's own store, against a loop of
oem_coverage_probs_device over the cells, with the cells cut into many chunks, against the (wrong) whole-store
binning, end to end into the cells EM, on errors, and at the size of one GPU's slice of BASELINE configs[4].
The per-cell kernels at bin, length and span edges: test_coverage_edges_gpu.py (grid: coverage_edges_common.py)."""
import os

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth
from oracle import c_oracle
from oracle import filter_py as fp
from tests.common import assert_counts_close

pytestmark = pytest.mark.gpu

RTOL = 1e-4  # north_star tolerance
THREADS = min(16, os.cpu_count() or 4)


def _join(cells):
    """Concatenates per-cell CSRs [(row_ptr from 0, tid)] into (cell_row_off, row_ptr, tid)."""
    cell_off, rps, tids, base = [0], [np.zeros(1, np.uint64)], [], 0
    for rp, tid in cells:
        rp = np.asarray(rp, dtype=np.uint64)
        rps.append(rp[1:] + np.uint64(base))
        tids.append(np.asarray(tid, dtype=np.uint32))
        base += int(rp[-1])
        cell_off.append(cell_off[-1] + len(rp) - 1)
    return np.array(cell_off, np.uint64), np.concatenate(rps), np.concatenate(tids)


def _slices(cell_off, row_ptr, c):
    r0, r1 = int(cell_off[c]), int(cell_off[c + 1])
    return r0, r1, int(row_ptr[r0]), int(row_ptr[r1])


def _per_cell_loop(cell_off, row_ptr, tid, s, e, tl, bin_width, model, growth, cells=None):
    """oem_coverage_probs_device on each cell's slice (row_ptr rebased to 0): the contract of the batched call."""
    out = np.full(len(tid), np.nan)
    L = _lib.lib()
    for c in range(len(cell_off) - 1) if cells is None else cells:
        r0, r1, a0, a1 = _slices(cell_off, row_ptr, c)
        rp = np.ascontiguousarray(row_ptr[r0:r1 + 1] - row_ptr[r0])
        got = np.zeros(max(a1 - a0, 1))
        _lib.check(L.oem_coverage_probs_device(rp.ctypes.data, tid[a0:a1].ctypes.data, s[a0:a1].ctypes.data,
                                               e[a0:a1].ctypes.data, tl.ctypes.data, r1 - r0, a1 - a0, len(tl),
                                               bin_width, model, growth, 0, got.ctypes.data))
        out[a0:a1] = got[:a1 - a0]
    return out


def _oracle(cell_off, row_ptr, tid, s, e, tl, bin_width, model, growth):
    want = np.zeros(len(tid))
    for c in range(len(cell_off) - 1):
        r0, r1, a0, a1 = _slices(cell_off, row_ptr, c)
        st = fp.Store(row_ptr=[int(x) - a0 for x in row_ptr[r0:r1 + 1]], tid=[int(x) for x in tid[a0:a1]],
                      start=[int(x) for x in s[a0:a1]], end=[int(x) for x in e[a0:a1]])
        want[a0:a1] = fp.coverage_probs(st, [int(x) for x in tl], bin_width, growth, model=model)
    return want


def _assert_close(got, want, median, what):
    """The tolerance of test_device_coverage_model_matches_the_oracle; NaN exactly where the reference has it."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    fin = ~np.isnan(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=2e-6, atol=1e-300, err_msg=what)
    rel = np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-300)
    assert np.median(rel) <= median, (what, np.median(rel))


def _oracle_cells(seed):
    """~12 cells over 60 transcripts: ten generated ones over transcripts 0..58, an empty cell among them, a
    one-read cell that is the only one to touch transcript 59, and some zero-span alignments."""
    T = 60
    cell_off, row_ptr, tid, _ = synth.make_cells(10, 120, T - 1, kbar=4.0, seed=seed)
    cells = []
    for c in range(10):
        r0, r1, a0, a1 = _slices(cell_off, row_ptr, c)
        cells.append((row_ptr[r0:r1 + 1] - row_ptr[r0], tid[a0:a1]))
    cells.insert(4, (np.zeros(1, np.uint64), np.zeros(0, np.uint32)))          # a cell without reads
    cells.append(([0, 2], [3, T - 1]))                                          # one read; the only user of T - 1
    cell_off, row_ptr, tid = _join(cells)
    tl, s, e = synth.make_coordinates(tid, T, seed=seed, zero_span_frac=0.02)
    assert np.count_nonzero(s == e) > 0
    return cell_off, row_ptr, tid, s, e, tl, T


@pytest.mark.parametrize("model,bin_width,growth", [("logistic", 100, 2.0), ("logistic", 40, 0.8),
                                                    ("binomial", 100, 2.0), ("binomial", 230, 2.0)])
def test_cells_match_the_oracle_cell_by_cell(model, bin_width, growth):
    """Each cell's part of the result is oracle/filter_py.coverage_probs on that cell's own store: bins of the
    cell's alignments only, probabilities and normalisation per cell (single_cell.rs:132-137)."""
    cell_off, row_ptr, tid, s, e, tl, T = _oracle_cells(seed=71 + bin_width)
    got = oarfish_amd.cells_coverage_probs(cell_off, row_ptr, tid, s, e, tl, bin_width=bin_width, model=model,
                                           growth_rate=growth)
    want = _oracle(cell_off, row_ptr, tid, s, e, tl, bin_width, model, growth)
    assert np.isnan(want).sum() > 0
    _assert_close(got, want, 1e-12 if model == "logistic" else 1e-9, f"{model} bw={bin_width}")
    sums = np.add.reduceat(np.nan_to_num(got), row_ptr[:-1].astype(np.int64))[np.diff(row_ptr) > 0]
    live = ~np.isnan(np.add.reduceat(got, row_ptr[:-1].astype(np.int64))[np.diff(row_ptr) > 0])
    np.testing.assert_allclose(sums[live], 1.0, rtol=1e-12)                    # normalised per read


def _loop_cells(n_cells=300, reads=2_000, T=5_000, seed=73):
    cell_off, row_ptr, tid, p = synth.make_cells(n_cells, reads, T, seed=seed, threads=THREADS)
    tl, s, e = synth.make_coordinates(tid, T, seed=seed, zero_span_frac=0.001, threads=THREADS)
    return cell_off, row_ptr, tid, p, s, e, tl, T


def test_cells_match_the_per_cell_loop():
    """~300 cells x 2 k reads over 5 k transcripts: the batched call against oem_coverage_probs_device per cell."""
    cell_off, row_ptr, tid, p, s, e, tl, T = _loop_cells()
    got = oarfish_amd.cells_coverage_probs(cell_off, row_ptr, tid, s, e, tl)
    want = _per_cell_loop(cell_off, row_ptr, tid, s, e, tl, 100, 1, 2.0)
    _assert_close(got, want, 1e-12, "batched vs loop")


def _plan(cell_off, row_ptr, tl, bin_width, budget):
    """The chunk rule of oem_coverage_cells.hip with only the bin budget binding: a cell's bins are bounded by
    min(all bins, alignments x widest transcript's bins); a chunk closes before the cell that would exceed it."""
    nb = np.ceil(tl.astype(np.float64) / bin_width).astype(np.int64)
    ub = [min(int(nb.sum()), int(row_ptr[cell_off[c + 1]] - row_ptr[cell_off[c]]) * int(nb.max()))
          for c in range(len(cell_off) - 1)]
    chunks, cur, n = 0, 0, 0
    for u in ub:
        if n and cur + u > budget:
            chunks, cur, n = chunks + 1, 0, 0
        cur, n = cur + u, n + 1
    return chunks + (n > 0), max(ub)


def test_chunking_is_invisible(monkeypatch):
    """With the bin budget of the testing build forcing many chunks -- one of them a single cell above the budget
    -- the result equals the one-chunk call up to the order of the atomic sums."""
    T = 2_000
    small = synth.make_cells(24, 20, T, seed=77)
    big = synth.make_cells(1, 2_000, T, seed=78)
    cells = []
    for co, rp, tid, _ in (small, big):
        for c in range(len(co) - 1):
            r0, r1, a0, a1 = _slices(co, rp, c)
            cells.append((rp[r0:r1 + 1] - rp[r0], tid[a0:a1]))
    cells.insert(9, cells.pop())                                                # the big cell among the small ones
    cell_off, row_ptr, tid = _join(cells)
    tl, s, e = synth.make_coordinates(tid, T, seed=77, zero_span_frac=0.01)
    one = oarfish_amd.cells_coverage_probs(cell_off, row_ptr, tid, s, e, tl)
    budget = 30_000
    n_chunks, largest = _plan(cell_off, row_ptr, tl, 100, budget)
    assert n_chunks >= 5 and largest > budget
    monkeypatch.setenv("OEM_COV_CELLS_CHUNK_BINS", str(budget))
    with _lib.testing():
        many = oarfish_amd.cells_coverage_probs(cell_off, row_ptr, tid, s, e, tl)
        many_log = oarfish_amd.cells_coverage_probs(cell_off, row_ptr, tid, s, e, tl, model="logistic")
    _assert_close(many, one, 1e-12, "chunks vs one chunk")
    _assert_close(many_log, oarfish_amd.cells_coverage_probs(cell_off, row_ptr, tid, s, e, tl, model="logistic"),
                  1e-12, "chunks vs one chunk (logistic)")


def test_cells_are_not_binned_together():
    """Binning the concatenation of all cells as one store (oem_coverage_probs_device on everything) mixes the
    coverage of every cell; the per-cell result must differ from it by far more than rounding."""
    cell_off, row_ptr, tid, p, s, e, tl, T = _loop_cells(n_cells=30, reads=1_000, T=2_000, seed=79)
    got = oarfish_amd.cells_coverage_probs(cell_off, row_ptr, tid, s, e, tl)
    whole = np.zeros(len(tid))
    _lib.check(_lib.lib().oem_coverage_probs_device(row_ptr.ctypes.data, tid.ctypes.data, s.ctypes.data, e.ctypes.data,
                                                    tl.ctypes.data, len(row_ptr) - 1, len(tid), T, 100, 1, 2.0, 0,
                                                    whole.ctypes.data))
    fin = ~np.isnan(got) & ~np.isnan(whole)
    rel = np.abs(got[fin] - whole[fin]) / np.maximum(np.abs(whole[fin]), 1e-300)
    assert np.mean(rel > 1e-6) > 0.5 and np.max(rel) > 1e-2, (np.mean(rel > 1e-6), np.max(rel))


def test_end_to_end_into_the_cells_em():
    """Coordinates -> cells_coverage_probs -> em_cells_sparse, against filter_py.coverage_probs + the oracle's
    em::em per cell (gate 50, 1000 iterations, 1e-3): the same kept columns, counts within the north star.  The
    zero-span alignments' NaN drops their reads on both sides (em.rs:115)."""
    n_cells, T = 6, 200
    cell_off, row_ptr, tid, p = synth.make_cells(n_cells, 800, T, kbar=5.0, seed=83)
    tl, s, e = synth.make_coordinates(tid, T, seed=83, zero_span_frac=0.005)
    cov = oarfish_amd.cells_coverage_probs(cell_off, row_ptr, tid, s, e, tl)
    indptr, cols, vals, infos = oarfish_amd.em_cells_sparse(cell_off, row_ptr, tid, p, cov, T, max_iter=1000,
                                                            convergence_thresh=1e-3)
    want_cov = _oracle(cell_off, row_ptr, tid, s, e, tl, 100, "binomial", 2.0)
    assert np.isnan(want_cov).sum() > 0
    for c in range(n_cells):
        r0, r1, a0, a1 = _slices(cell_off, row_ptr, c)
        o = c_oracle.Store(row_ptr[r0:r1 + 1] - row_ptr[r0], tid[a0:a1], p[a0:a1], want_cov[a0:a1], T)
        want, wi = c_oracle.do_em(o, max_iter=1000, conv_thresh=1e-3, min_iter_gate=50)
        assert abs(infos[c].niter - wi.niter) <= 1, (c, infos[c], wi.niter)
        sl = slice(int(indptr[c]), int(indptr[c + 1]))
        got = np.zeros(T)
        got[cols[sl]] = vals[sl]
        if infos[c].niter == wi.niter:
            np.testing.assert_array_equal(cols[sl], np.nonzero(want > 0.0)[0], err_msg=f"cell {c}")
        assert_counts_close(got, want, r1 - r0, T, RTOL, f"cell {c}")


def test_an_alignment_past_its_transcript_names_the_cell():
    """add_interval's range check (oarfish_types.rs:504-505): OEM_ERR_STATE whose message names the first cell
    that has such an alignment; the next call in the same process works."""
    cell_off, row_ptr, tid, s, e, tl, T = _oracle_cells(seed=89)
    bad_cell = 6
    _, _, a0, a1 = _slices(cell_off, row_ptr, bad_cell)
    e_bad = e.copy()
    j = a0 + (a1 - a0) // 2
    e_bad[j] = np.uint32(int(tl[tid[j]]) + 500)
    with pytest.raises(oarfish_amd.OemError) as ei:
        oarfish_amd.cells_coverage_probs(cell_off, row_ptr, tid, s, e_bad, tl)
    assert ei.value.code == _lib.OEM_ERR_STATE
    assert f"cell {bad_cell}:" in str(ei.value) and "outside its transcript" in str(ei.value)
    got = oarfish_amd.cells_coverage_probs(cell_off, row_ptr, tid, s, e, tl)
    want = _per_cell_loop(cell_off, row_ptr, tid, s, e, tl, 100, 1, 2.0)
    _assert_close(got, want, 1e-12, "after an error")


def test_c5_slice_of_one_gpu():
    """One GPU's slice of BASELINE configs[4] (625 cells x 50 k reads over 60 k transcripts): one call, checked
    against oem_coverage_probs_device on 16 sampled cells."""
    n_cells, T = 625, 60_000
    cell_off, row_ptr, tid, _ = synth.make_cells(n_cells, 50_000, T, seed=37, threads=THREADS)
    tl, s, e = synth.make_coordinates(tid, T, seed=37, zero_span_frac=0.001, threads=THREADS)
    got = oarfish_amd.cells_coverage_probs(cell_off, row_ptr, tid, s, e, tl)
    cells = np.random.default_rng(3).choice(n_cells, 16, replace=False)
    want = _per_cell_loop(cell_off, row_ptr, tid, s, e, tl, 100, 1, 2.0, cells=cells)
    for c in cells:
        _, _, a0, a1 = _slices(cell_off, row_ptr, c)
        _assert_close(got[a0:a1], want[a0:a1], 1e-12, f"cell {c}")
