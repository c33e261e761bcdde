"""GPU tests of the per-cell session (oem_cells_stream_*, oarfish_amd.CellsStream): cells pushed one by one, from
several threads, in any order, against the oracle's em::em on every cell's own store (single_cell.rs:139-160) -- the
bar tests/test_cells_paths_gpu.py holds the one-call entry points to, on the same fixtures."""
import ctypes as C
import threading

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib
from tests.common import assert_cell_matches_oracle
from tests.test_cells_paths_gpu import COV, DECLINE, MAX_ITER, T, _cell, _check, _run, declining, plain  # noqa: F401
from tests.test_cells_sparse_gpu import _check_structure

pytestmark = pytest.mark.gpu


def _cell_arrays(fx, c):
    r0, r1, a0, a1 = _cell(fx, c)
    return (fx["row_ptr"][r0:r1 + 1] - fx["row_ptr"][r0], fx["tid"][a0:a1], fx["p"][a0:a1], fx["s"][a0:a1], fx["e"][a0:a1])


def _coverage(fx):
    return dict(COV, txp_len=fx["tl"])


def _push_all(cs, fx, coverage, n_threads=4, seed=7):
    """Every cell of the fixture, in a shuffled order, from n_threads threads; returns ticket -> fixture cell."""
    n = len(fx["cell_off"]) - 1
    order = np.random.default_rng(seed).permutation(n)
    cell_of_ticket, errors = {}, []
    lock = threading.Lock()

    def work(k):
        try:
            for c in order[k::n_threads]:
                rp, tid, p, s, e = _cell_arrays(fx, int(c))
                t = cs.push(rp, tid, p, s, e) if coverage else cs.push(rp, tid, p)
                with lock:
                    assert t not in cell_of_ticket
                    cell_of_ticket[t] = int(c)
        except BaseException as ex:   # noqa: BLE001 - reported by the main thread
            errors.append(ex)

    th = [threading.Thread(target=work, args=(k,)) for k in range(n_threads)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    assert sorted(cell_of_ticket) == list(range(n))
    return cell_of_ticket


def _check_result(got, fx, cell_of_ticket, coverage, label):
    """Result cell k is the cell with ticket k: held to the oracle's answer for that fixture cell."""
    indptr, cols, vals, infos = got
    n = len(cell_of_ticket)
    _check_structure(indptr, cols, vals, n, T)
    assert len(infos) == n, label
    want = fx["want"][MAX_ITER] if coverage else _want_plain(fx)
    reads = np.diff(fx["cell_off"].astype(np.int64))
    for k in range(n):
        c = cell_of_ticket[k]
        s = slice(int(indptr[k]), int(indptr[k + 1]))
        assert_cell_matches_oracle(infos[k], want[c], int(reads[c]), T, f"{label}: ticket {k} (cell {c})", cols=cols[s],
                                   vals=vals[s])


_PLAIN_WANT = {}


def _want_plain(fx):
    """em::em without a coverage column (w = as_prob) on every cell's own store, once per fixture."""
    from oracle import c_oracle
    key = id(fx)
    if key not in _PLAIN_WANT:
        out = []
        for c in range(len(fx["cell_off"]) - 1):
            rp, tid, p, _, _ = _cell_arrays(fx, c)
            o = c_oracle.Store(rp, tid, p, None, T)
            out.append(c_oracle.do_em(o, max_iter=MAX_ITER, conv_thresh=1e-3, min_iter_gate=50))
        _PLAIN_WANT[key] = out
    return _PLAIN_WANT[key]


def test_shuffled_pushes_from_four_threads(plain):
    with oarfish_amd.CellsStream(T, max_iter=MAX_ITER, conv_thresh=1e-3) as cs:
        tickets = _push_all(cs, plain, coverage=False)
        got = cs.finish()
        info = cs.info()
    _check_result(got, plain, tickets, False, "stream")
    nnz = len(plain["tid"])
    assert info["cells"] == len(tickets) and info["alignments"] == nnz and info["groups"] == 1 and info["groups_batched"] == 1


def test_shuffled_pushes_with_the_coverage_model(plain):
    with oarfish_amd.CellsStream(T, max_iter=MAX_ITER, conv_thresh=1e-3, coverage=_coverage(plain)) as cs:
        tickets = _push_all(cs, plain, coverage=True)
        got = cs.finish()
    _check_result(got, plain, tickets, True, "stream/coverage")


@pytest.mark.parametrize("coverage", [False, True])
def test_many_groups_under_back_pressure(plain, coverage):
    nnz = np.diff(plain["row_ptr"][plain["cell_off"].astype(np.int64)].astype(np.int64))
    budget = int(np.sort(nnz)[-2:].sum()) - 1      # smaller than the two largest cells together
    with oarfish_amd.CellsStream(T, max_iter=MAX_ITER, conv_thresh=1e-3, coverage=_coverage(plain) if coverage else None,
                                 group_cells=3, max_staged_nnz=budget) as cs:
        tickets = _push_all(cs, plain, coverage=coverage)
        before = cs.info()
        got = cs.finish()
        info = cs.info()
    _check_result(got, plain, tickets, coverage, f"stream/groups cov={coverage}")
    print("stream info:", before, info)
    assert info["groups"] > 1 and info["groups"] >= len(tickets) // 3
    assert info["groups_before_finish"] >= 1 and before["groups"] >= 1


@pytest.mark.parametrize("coverage", [False, True])
def test_the_declined_group_falls_back_cell_by_cell(declining, coverage):
    """The tiler refuses the batch that holds the declining cell: the session's group runs cell by cell, over the
    resident CSR the store hands back."""
    with oarfish_amd.CellsStream(T, max_iter=MAX_ITER, conv_thresh=1e-3,
                                 coverage=_coverage(declining) if coverage else None) as cs:
        tickets = _push_all(cs, declining, coverage=coverage)
        got = cs.finish()
        info = cs.info()
    assert info["groups"] == 1 and info["groups_batched"] == 0, info
    _check_result(got, declining, tickets, coverage, f"stream/decline cov={coverage}")


def test_host_layout_builder_from_a_session(plain, monkeypatch):
    """The device layout builder declines (forced in the test-only library): the host builder gets the group's
    concatenated row pointers, which the session makes only then."""
    monkeypatch.setenv("OEM_TEST_HOST_LAYOUT", "1")
    with _lib.testing():
        with oarfish_amd.CellsStream(T, max_iter=MAX_ITER, conv_thresh=1e-3) as cs:
            tickets = _push_all(cs, plain, coverage=False)
            got = cs.finish()
            info = cs.info()
    assert info["groups_batched"] == 1
    _check_result(got, plain, tickets, False, "stream/host layout")


def test_a_rejected_cell_uses_no_ticket(plain):
    n = len(plain["cell_off"]) - 1
    with oarfish_amd.CellsStream(T, max_iter=MAX_ITER, conv_thresh=1e-3, coverage=_coverage(plain)) as cs:
        tickets = {}
        for c in range(n):
            rp, tid, p, s, e = _cell_arrays(plain, c)
            if c == 3:
                bad = tid.copy()
                bad[-1] = T
                with pytest.raises(oarfish_amd.OemError) as ei:
                    cs.push(rp, bad, p, s, e)
                assert ei.value.code == _lib.OEM_ERR_ARG and "n_txps" in str(ei.value)
            if c == 6:
                bad = rp.copy()
                bad[2], bad[3] = rp[3] + 1, rp[2]
                assert bad[3] < bad[2]
                with pytest.raises(oarfish_amd.OemError) as ei:
                    cs.push(bad, tid, p, s, e)
                assert ei.value.code == _lib.OEM_ERR_ARG and "non-decreasing" in str(ei.value)
            if c == 8:
                with pytest.raises(oarfish_amd.OemError) as ei:
                    cs.push(rp, tid, p)
                assert ei.value.code == _lib.OEM_ERR_ARG and "aln_start" in str(ei.value)
            tickets[cs.push(rp, tid, p, s, e)] = c
        assert sorted(tickets) == list(range(n)) and cs.info()["cells"] == n
        got = cs.finish()
    _check_result(got, plain, tickets, True, "stream/rejected")


def test_state_errors_and_the_empty_session(plain):
    with oarfish_amd.CellsStream(T, max_iter=MAX_ITER) as cs:
        indptr, cols, vals, infos = cs.finish()
        assert list(indptr) == [0] and len(cols) == 0 and len(vals) == 0 and infos == []
        assert cs.info()["cells"] == 0 and cs.info()["groups"] == 0
        with pytest.raises(oarfish_amd.OemError) as ei:
            cs.finish()
        assert ei.value.code == _lib.OEM_ERR_STATE
        rp, tid, p, _, _ = _cell_arrays(plain, 2)
        with pytest.raises(oarfish_amd.OemError) as ei:
            cs.push(rp, tid, p)
        assert ei.value.code == _lib.OEM_ERR_STATE
    with oarfish_amd.CellsStream(T, max_iter=MAX_ITER) as cs:
        t = cs.push(rp, tid, p)
        got = cs.finish()
        with pytest.raises(oarfish_amd.OemError) as ei:
            cs.finish()
        assert ei.value.code == _lib.OEM_ERR_STATE
    _check_result(got, plain, {t: 2}, False, "stream/one cell")


def test_destroy_before_finish_is_an_orderly_cancel(plain):
    """A session dropped with a group on the device and cells still staged: destroy returns, and the device serves
    the next call."""
    cs = oarfish_amd.CellsStream(T, max_iter=MAX_ITER, conv_thresh=1e-3, group_cells=3)
    _push_all(cs, plain, coverage=False)
    assert cs.info()["groups"] >= 1
    cs.close()
    got = _run("sparse", plain, MAX_ITER)
    _check("sparse", got, plain, MAX_ITER, "after a cancelled session")
