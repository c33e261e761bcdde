"""GPU tests of the coverage model at bin, length and span edges: the whole-store kernels (oem_coverage_device.hip:
oem_coverage_probs_device, oem_store_create_coverage) and the per-cell ones (oem_coverage_cells.hip:
oem_coverage_probs_cells_device) against oracle/filter_py.coverage_probs on the grid of coverage_edges_common.py --
one-bin transcripts, transcripts shorter than the bin width, exact multiples, rounded bin widths above and below the
exact one, stop == len and stop == len + 1, start > end, zero spans, bin width 1, a length f32 cannot hold, both
logistic clamps.  test_coverage_edges.py shows on the CPU that the grid holds each of these and that the oracle does
not depend on the summation order on it, so a difference above the bounds here is not the atomics' order.

Bounds (test_cells_coverage_gpu._assert_close): NaN in exactly the oracle's places, rtol 2e-6, median relative
error 1e-12 (logistic) or 1e-9 (binomial); on the power-of-two geometries the logistic maximum is 1e-12."""
import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib
from oarfish_amd.types import DeviceStore
from oracle import c_oracle
from oracle import filter_py as fp
from tests import coverage_edges_common as ce
from tests.common import assert_counts_close

pytestmark = pytest.mark.gpu

CASES = [("logistic", ce.GROWTH), ("logistic", ce.GROWTH_LARGE), ("binomial", ce.GROWTH)]


def _cov_device(g, width, model, growth):
    out = np.empty(g.nnz)
    _lib.check(_lib.lib().oem_coverage_probs_device(g.row_ptr.ctypes.data, g.tid.ctypes.data, g.start.ctypes.data,
                                                    g.end.ctypes.data, g.tl.ctypes.data, g.n_reads, g.nnz, g.n_txps,
                                                    width, ce.MODELS[model], growth, 0, out.ctypes.data))
    return out


@pytest.mark.parametrize("width", ce.WIDTHS)
@pytest.mark.parametrize("model,growth", CASES)
def test_whole_store_kernels_match_the_oracle(model, growth, width):
    g = ce.store(width)
    got = _cov_device(g, width, model, growth)
    ce.assert_device_close(got, ce.oracle(width, model, growth), model, f"whole store, width {width}, {model} {growth}",
                           exact_reads=ce.pow2_reads(g))


@pytest.mark.parametrize("coding", [0, 2])
@pytest.mark.parametrize("model", ["logistic", "binomial"])
def test_store_with_coverage_on_the_width_100_grid(model, coding):
    """DeviceStore.with_coverage on the width-100 store: the returned column under the same comparison, then five EM
    iterations against the oracle's em::em on the ORACLE's column.  A NaN read is dropped on both sides (em.rs:115),
    so the mass is the number of reads without a NaN.

    Bound of the EM comparison.  The device's weights differ from the oracle's by delta relative: the column's
    largest relative error (measured here, at most the 2e-6 asserted first), plus 2^-24 for weight_coding 2 (the
    product rounded once to f32).  One iteration maps weights and abundances that are off by (delta, eps) to
    abundances off by at most 2 (delta + eps): each term theta_t w_t / sum(theta w) is a ratio of two positive
    sums.  From equal starts, eps_5 <= (2 + 4 + 8 + 16 + 32) delta = 62 delta; 1e-10 on top for the order of the
    sums (the bound the suite uses where only the order differs)."""
    width = 100
    g = ce.store(width)
    want_cov = ce.oracle(width, model, ce.GROWTH)
    store, cov = DeviceStore.with_coverage(g.row_ptr, g.tid, g.as_prob, g.start, g.end, g.tl, bin_width=width,
                                           model=model, growth_rate=ce.GROWTH, weight_coding=coding,
                                           return_coverage=True)
    with store:
        ce.assert_device_close(cov, want_cov, model, f"with_coverage column, {model}, coding {coding}")
        got, info = store.em_run(max_iter=5, conv_thresh=0.0, min_iter_gate=50)
    rel, _ = ce.rel_err(cov, want_cov)
    o = c_oracle.Store(g.row_ptr, g.tid, g.as_prob, want_cov, g.n_txps)
    want, wi = c_oracle.do_em(o, max_iter=5, conv_thresh=0.0, min_iter_gate=50)
    assert info.niter == wi.niter == 5
    nan_reads = int(np.isnan(want_cov).reshape(-1, 2).any(axis=1).sum())
    live = g.n_reads - nan_reads
    assert nan_reads > 0 and abs(want.sum() - live) < 1e-9 * live and abs(got.sum() - live) < 1e-9 * live
    bound = 62 * (rel.max() + (2.0 ** -24 if coding == 2 else 0.0)) + 1e-10
    print(f"EM after with_coverage, {model}, coding {coding}: bound {bound:.3e}, worst "
          f"{np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)):.3e}")
    assert_counts_close(got, want, g.n_reads, g.n_txps, bound, f"EM on the fused store, {model}, coding {coding}")


@pytest.mark.parametrize("width", ce.WIDTHS)
@pytest.mark.parametrize("model", ["logistic", "binomial"])
def test_per_cell_kernels_match_the_oracle_cell_by_cell(model, width, monkeypatch):
    """cells_coverage_probs on the cells layout (a cell per geometry, an empty cell, and a last cell that reuses a
    transcript with other alignments) against the oracle on each cell's own store: once as is, once with the bin
    budget of the test-only library at 1, which closes a chunk before every cell that has alignments."""
    cl = ce.cells(width)
    g = cl.grid
    want = ce.cells_oracle(width, model, ce.GROWTH)
    args = (cl.cell_off, g.row_ptr, g.tid, g.start, g.end, g.tl)
    kw = dict(bin_width=width, model=model, growth_rate=ce.GROWTH)
    one = oarfish_amd.cells_coverage_probs(*args, **kw)
    monkeypatch.setenv("OEM_COV_CELLS_CHUNK_BINS", "1")
    with _lib.testing():
        many = oarfish_amd.cells_coverage_probs(*args, **kw)
    for what, got in (("one chunk", one), ("a chunk per cell", many)):
        ce.assert_device_close(got, want, model, f"cells, width {width}, {model}, {what}", exact_reads=ce.pow2_reads(g))
        a, b = cl.pair_columns(got)
        wa, wb = cl.pair_columns(want)
        for x, w in ((a, wa), (b, wb)):                       # each cell of the pair equals its own oracle ...
            fin = ~np.isnan(w)
            np.testing.assert_allclose(x[fin], w[fin], rtol=2e-6, atol=1e-300, err_msg=what)
        if cl.pair_can_differ(model):                          # ... and the two differ: the bins are per cell
            fin = ~np.isnan(wa)
            assert np.any(np.abs(a[fin] - b[fin]) > 1e-3 * np.abs(a[fin])), (width, model, what)


# ---- errors: an end bin past the last bin ----------------------------------------------------------------------------
def _error_layout(bad):
    """Two cells over the geometries (1, 100) and (200, 100), each with its own grid alignments; `bad` = (geometry,
    start, stop) is added to its geometry's cell, or None."""
    geoms = [(1, 100), (200, 100)]
    cells = [[(gi, s, e, k) for s, e, k in ce.alignments(*geom)] for gi, geom in enumerate(geoms)]
    if bad is not None:
        cells[bad[0]].insert(1, (bad[0], bad[1], bad[2], ce.PAST_END))
    g = ce.Grid(geoms, [x for c in cells for x in c])
    cell_off = np.concatenate([[0], np.cumsum([len(c) for c in cells])]).astype(np.uint64)
    return g, cell_off


@pytest.mark.parametrize("bad", [(0, 0, 2), (1, 0, 301)], ids=["one bin", "multiple of the width"])
def test_an_end_bin_past_the_last_bin_is_an_error(bad):
    """add_interval's slice [start_bin..end_bin] panics when end_bin > n (oarfish_types.rs:515): both whole-store
    entry points and the per-cell call return OEM_ERR_STATE with "outside its transcript" (a flag the kernels set;
    cov_add_interval returns before its bin loop), and a good call afterwards passes."""
    width = 100
    tlen = [1, 200][bad[0]]
    assert ce.end_bin_of_add_interval(bad[2], tlen, width) > ce.n_bins(tlen, width)
    g, cell_off = _error_layout(bad)
    with pytest.raises(oarfish_amd.OemError) as raw:
        _cov_device(g, width, "logistic", ce.GROWTH)
    with pytest.raises(oarfish_amd.OemError) as fused:
        DeviceStore.with_coverage(g.row_ptr, g.tid, g.as_prob, g.start, g.end, g.tl, bin_width=width)
    with pytest.raises(oarfish_amd.OemError) as per_cell:
        oarfish_amd.cells_coverage_probs(cell_off, g.row_ptr, g.tid, g.start, g.end, g.tl, bin_width=width)
    for ei in (raw, fused, per_cell):
        assert ei.value.code == _lib.OEM_ERR_STATE and "outside its transcript" in str(ei.value)
    assert str(raw.value) == str(fused.value) and f"cell {bad[0]}:" in str(per_cell.value)
    good, good_off = _error_layout(None)
    st = good.fp_store()
    want = np.asarray(fp.coverage_probs(st, good.txp_len, width, ce.GROWTH, model="logistic"))
    ce.assert_device_close(_cov_device(good, width, "logistic", ce.GROWTH), want, "logistic", "after an error")
    got = oarfish_amd.cells_coverage_probs(good_off, good.row_ptr, good.tid, good.start, good.end, good.tl,
                                           bin_width=width, model="logistic", growth_rate=ce.GROWTH)
    ce.assert_device_close(got, want, "logistic", "cells after an error")   # the cells share no transcript
    with DeviceStore.with_coverage(good.row_ptr, good.tid, good.as_prob, good.start, good.end, good.tl,
                                   bin_width=width) as d:
        d.em_run(max_iter=3)
