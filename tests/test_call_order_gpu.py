"""GPU tests of the order of calls on one oem_store handle: a call's result must not depend on the calls made before
it on the same handle (tests/call_order_common.py has the alphabet of operations, the walk and the references).

  test_every_ordered_pair[A|B]   one handle of the test-only library, the whole alphabet: the Euler walk performs every
                                 ordered pair of operations (self pairs included) as neighbours exactly once, and after
                                 every step the result is held to the oracle and to the same operation on a fresh
                                 handle.  The executed pair set is asserted to be the full set.
  test_two_handles_interleaved   product library, the knob-free operations: handles of A and B open together, their
                                 walks alternating step by step; every 25 steps a per-cell sparse EM of 12 ragged cells
                                 and a records -> store call run in between (the library's global upload lanes and
                                 worker threads), each against its own existing reference.
  test_named_pairs               the pairs the code makes riskiest (call_order_common.PAIRS), each on a fresh handle.

A failure names (step index, previous operation, operation, store).

Float counts against the fresh handle: one-pass operations 1e-12; multi-iteration operations ten times the run-to-run
noise measured between two fresh handles when the module's references are built (printed per operation; run with -s),
never above the operation's oracle tolerance (1e-9 for the 40-iteration runs, 1e-8 for converged
runs and replicates).  Measured on an MI355X (both libraries, both stores; the
figures move by a few 1e-15 from run to run, so the module measures them again each time it builds its references):
  one pass (m_step, m_step_weighted, em_zero)              floor 4.4e-16 .. 6.3e-16, allowed 1e-12 (the project's number)
  40 iterations (em_40, em_40_classic, em_init, history_8)  floor 3.5e-15 .. 4.8e-15, allowed 3.5e-14 .. 4.8e-14
  converged runs (em_converged, em_converged_graph)         floor 4.8e-15 .. 8.4e-15, allowed 4.8e-14 .. 8.4e-14
  replicates (boot_*, history_500)                          floor 5.2e-15 .. 1.0e-14, allowed 5.2e-14 .. 1.0e-13
The worst figure any step of the walks showed against its fresh handle was 1.0e-14 (each walk prints its own: -s)."""
import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth
from oarfish_amd.types import DeviceStore
from tests import call_order_common as co
from tests.common import assert_cell_matches_oracle

pytestmark = pytest.mark.gpu

_KNOBS = sorted({k for op in co.OPS for k in op.knobs})


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    """the operations set and remove their own knobs: none may come in from outside"""
    for k in _KNOBS + ["OEM_TILE_NT", "OEM_FOLD_NT", "OEM_WINDOW_CAP", "OEM_NO_DICT", "OEM_DICT_NO_FUSE"]:
        monkeypatch.delenv(k, raising=False)


_fresh = {}


def fresh(store, library):
    """The fresh-handle references of (store, library), built once."""
    key = (store, library)
    if key not in _fresh:
        fx = co.fixture(store)
        if library == "testing":
            with _lib.testing():
                _fresh[key] = co.fresh_ref(fx, co.OPS)
        else:
            _fresh[key] = co.fresh_ref(fx, co.KNOB_FREE)
    return _fresh[key]


def _check_shape(d, store):
    if store == "A":       # what makes A the store it is chosen for: asserted, not assumed
        assert d.info(_lib.OEM_INFO_TILES) >= 2
        assert d.info(_lib.OEM_INFO_REMOTE_ALIGNMENTS) > 0
    else:
        assert d.info(_lib.OEM_INFO_TILES) >= 1


def _print_worst(store, ref):
    for (s, name), w in sorted(co.WORST.items()):
        if s == store and name in ref:
            print(f"store {s}, {name}: worst figure of a used handle against the fresh one {w:.3e} (floor {ref[name][1]:.3e}, "
                  f"allowed {ref[name][2]:.3e})")


@pytest.mark.parametrize("store", co.STORES)
def test_every_ordered_pair(store):
    fx = co.fixture(store)
    ref = fresh(store, "testing")
    n = len(co.OPS)
    executed = set()
    co.WORST.clear()
    with _lib.testing(), co.open_store(fx) as d:
        _check_shape(d, store)
        steps = sum(1 for _ in co.walk(d, fx, co.OPS, ref, executed))
    _print_worst(store, ref)
    assert steps == n * n + 1
    assert executed == {(a, b) for a in range(n) for b in range(n)}


# ---- the calls between the walks: their own references, computed once ----------------------------------------------------
_between = {}


def _cells_reference():
    if "cells" not in _between:
        from tests.test_tile_instantiations_gpu import CELL_ITER, CELL_READS, CELL_T, _cell_reference, _cell_weights, _cells
        cell_off, row_ptr, tid, _ = _cells()
        p, _cov = _cell_weights("coded")
        _between["cells"] = (cell_off, row_ptr, tid, p, CELL_T, CELL_ITER, CELL_READS, _cell_reference("coded"))
    return _between["cells"]


def _records_reference():
    if "records" not in _between:
        st = synth.make_store(3_000, 200, seed=411)
        _between["records"] = synth.make_records(st, seed=412)
    return _between["records"]


def _a_cells_call(what):
    cell_off, row_ptr, tid, p, T, n_iter, reads, want = _cells_reference()
    indptr, cols, vals, infos = oarfish_amd.em_cells_sparse(cell_off, row_ptr, tid, p, None, T, max_iter=n_iter,
                                                            convergence_thresh=1e-3)
    assert len(indptr) == len(reads) + 1 and int(indptr[-1]) == len(cols) == len(vals)
    for c, n in enumerate(reads):
        s = slice(int(indptr[c]), int(indptr[c + 1]))
        assert_cell_matches_oracle(infos[c], want[c], n, T, f"{what}: cell {c}", cols=cols[s], vals=vals[s])


def _a_records_call(what):
    sr = _records_reference()
    one, kept, dt = DeviceStore.from_records(sr.filters, sr.txp_len, sr.records, sr.group_off)
    with one:
        assert np.array_equal(kept, sr.kept) and dt == sr.discard, what
        assert (one.n_reads, one.nnz, one.n_txps) == (np.count_nonzero(sr.kept), int(sr.kept.sum()), len(sr.txp_len)), what


def test_two_handles_interleaved():
    ops = co.KNOB_FREE
    n = len(ops)
    fxs = {s: co.fixture(s) for s in co.STORES}
    refs = {s: fresh(s, "product") for s in co.STORES}
    executed = {s: set() for s in co.STORES}
    co.WORST.clear()
    with co.open_store(fxs["A"]) as da, co.open_store(fxs["B"]) as db:
        _check_shape(da, "A")
        _check_shape(db, "B")
        walks = [co.walk(da, fxs["A"], ops, refs["A"], executed["A"]), co.walk(db, fxs["B"], ops, refs["B"], executed["B"])]
        for i in range(n * n + 1):
            for w in walks:
                assert next(w) == i
            if i % 25 == 24:
                _a_cells_call(f"between steps {i} and {i + 1}")
                _a_records_call(f"between steps {i} and {i + 1}")
        for w in walks:
            assert next(w, None) is None
    for s in co.STORES:
        _print_worst(s, refs[s])
        assert executed[s] == {(a, b) for a in range(n) for b in range(n)}, s


@pytest.mark.parametrize("a,b", co.PAIRS, ids=[f"{a}->{b}" for a, b in co.PAIRS])
def test_named_pairs(a, b):
    for store in co.STORES:
        ref = fresh(store, "testing")
        with _lib.testing():
            co.run_pair(store, a, b, ref)
