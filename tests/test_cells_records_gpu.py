"""GPU tests of the per-cell calls' records form (oem_em_run_cells_records_sparse, the records session): cells go from
their alignment records to their entries in one device call.  The filter side is held to the host builder cell by cell
(kept, discard tables, the filtered CSR byte for byte), the EM side to the oracle's em::em on every cell's own store as
the host builder exports it -- the bar of tests/test_cells_paths_gpu.py, not another call that shares the path."""
import ctypes as C
import threading

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth
from oarfish_amd.builder import ALN_RECORD, StoreBuilder
from oracle import c_oracle
from oracle import filter_py as fp
from tests import filter_common as fc
from tests.common import assert_cell_matches_oracle
from tests.test_cells_paths_gpu import _last_paths
from tests.test_cells_sparse_gpu import _check_structure

pytestmark = pytest.mark.gpu

T = 600                # as tests/test_cells_paths_gpu.py
MAX_ITER = 60          # with em::em's gate of 50: some cells converge, the others stop at max_iter
COVS = {-1: None, 0: dict(bin_width=100, model="logistic", growth_rate=2.0), 1: dict(bin_width=100, model="binomial", growth_rate=2.0)}
KEEP = "OEM_TEST_KEEP_RECORDS_CSR"


# ---- cells as pieces: [(records, group_off from 0)] ------------------------------------------------------------------
def _concat(pieces):
    """(records, group_off, cell_group_off) of the cells one after the other."""
    recs = [r for r, _ in pieces] or [np.zeros(0, dtype=ALN_RECORD)]
    goffs, cgo, base = [np.zeros(1, dtype=np.uint64)], [0], 0
    for r, g in pieces:
        goffs.append(np.asarray(g[1:], dtype=np.uint64) + np.uint64(base))
        base += len(r)
        cgo.append(cgo[-1] + len(g) - 1)
    return np.concatenate(recs), np.concatenate(goffs), np.array(cgo, dtype=np.uint64)


def _split(records, group_off, cell_group_off):
    out = []
    for c in range(len(cell_group_off) - 1):
        g0, g1 = int(cell_group_off[c]), int(cell_group_off[c + 1])
        r0, r1 = int(group_off[g0]), int(group_off[g1])
        out.append((records[r0:r1].copy(), group_off[g0:g1 + 1] - group_off[g0]))
    return out


def _host_way(filters, txp_len, pieces):
    """The long way round, per cell: a builder of its own, add_groups over the cell's groups, export, discard table."""
    out = []
    for rec, goff in pieces:
        with StoreBuilder(filters, txp_len) as b:
            kept = b.add_groups(rec, goff)
            rp, tid, p, s, e, _ = b.export()
            out.append(dict(kept=kept, rp=rp, tid=tid, p=p, s=s, e=e, table=b.discard_table()))
    return out


def _oracle(host, txp_len, n_txps, model, max_iter=MAX_ITER):
    """em::em on every cell's exported store; for models 0 / 1 over filter_py's coverage column of that store."""
    want = []
    for h in host:
        cov = None
        if model >= 0:
            st = fp.Store(row_ptr=[int(x) for x in h["rp"]], tid=[int(x) for x in h["tid"]], start=[int(x) for x in h["s"]],
                          end=[int(x) for x in h["e"]])
            cov = np.asarray(fp.coverage_probs(st, [int(x) for x in txp_len], COVS[model]["bin_width"], COVS[model]["growth_rate"],
                                               model=COVS[model]["model"]), dtype=np.float64)
        o = c_oracle.Store(h["rp"], h["tid"], h["p"], cov, n_txps)
        want.append(c_oracle.do_em(o, max_iter=max_iter, conv_thresh=1e-3, min_iter_gate=50))
    return want


def _check_filter_side(got, host, label):
    kept, tables = got[4], got[5]
    assert len(tables) == len(host), label
    g = 0
    for c, h in enumerate(host):
        n = len(h["kept"])
        assert np.array_equal(kept[g:g + n], h["kept"]), f"{label}: kept of cell {c}"
        assert tables[c] == h["table"], f"{label}: discard table of cell {c}: {tables[c]} != {h['table']}"
        g += n
    assert g == len(kept), label


def _check_em_side(got, host, want, n_txps, label):
    indptr, cols, vals, infos = got[:4]
    n = len(host)
    _check_structure(indptr, cols, vals, n, n_txps)
    assert len(infos) == n, label
    for c in range(n):
        s = slice(int(indptr[c]), int(indptr[c + 1]))
        assert_cell_matches_oracle(infos[c], want[c], len(host[c]["rp"]) - 1, n_txps, f"{label}: cell {c}", cols=cols[s],
                                   vals=vals[s])


def _run(filters, txp_len, pieces, model=-1, max_iter=MAX_ITER):
    rec, goff, cgo = _concat(pieces)
    return oarfish_amd.em_cells_records_sparse(filters, txp_len, rec, goff, cgo, coverage=COVS[model], max_iter=max_iter,
                                               conv_thresh=1e-3)


# ---- fixture 1: many small cells ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_cells():
    return _small_cells()


def _small_cells():
    F, txp_len, groups = fc.random_groups(31, 4000, T=120)
    rng = np.random.default_rng(5)
    sizes = [int(rng.integers(0, 6)) for _ in range(200)]
    rest = len(groups) - sum(sizes)
    cuts = np.sort(rng.integers(0, rest, 6))
    sizes += [int(x) for x in np.diff(np.concatenate([[0], cuts, [rest]]))]
    cgo = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    rec, goff = fc.pack(groups)
    pieces = _split(rec, goff, cgo)
    filters = fc.filters_dict(F)
    host = _host_way(filters, txp_len, pieces)
    # the fixture is what it is meant to be: wavefronts that span many cells, empty cells, cells that keep nothing
    assert len(pieces) == 207 and sum(1 for _, g in pieces if len(g) == 1) == 34
    assert sum(1 for h in host if len(h["kept"]) and not h["kept"].any()) == 139
    assert sum(int((h["kept"] > 0).sum()) for h in host) == 184
    nz = {k: sum(1 for h in host if h["table"][k]) for k in host[0]["table"]}
    assert len(nz) == 10 and all(v >= 1 for v in nz.values()) and nz["discard_score"] == 1, nz
    return dict(filters=filters, txp_len=np.asarray(txp_len, dtype=np.uint64), pieces=pieces, host=host, T=120)


@pytest.mark.parametrize("chunk", [1, 64, None])
def test_kept_and_discard_tables_of_many_small_cells(small_cells, chunk, monkeypatch):
    fx = small_cells
    if chunk is not None:
        monkeypatch.setenv("OEM_FILTER_CHUNK_GROUPS", str(chunk))
    with _lib.testing():
        got = _run(fx["filters"], fx["txp_len"], fx["pieces"], max_iter=5)
    _check_filter_side(got, fx["host"], f"small cells, chunk {chunk}")
    if chunk is None:   # ... and the product library
        _check_filter_side(_run(fx["filters"], fx["txp_len"], fx["pieces"], max_iter=5), fx["host"], "small cells (product)")


def _kept_csr(L):
    dims = (C.c_uint64 * 3)()
    _lib.check(L.oem_debug_cells_records_last_csr(dims, None, None, None, None, None, None))
    R, nnz, nc = (int(x) for x in dims)
    rp = np.zeros(R + 1, dtype=np.uint32)
    tid, p, s, e = (np.zeros(nnz, dtype=np.uint32) for _ in range(4))
    cro = np.zeros(nc + 1, dtype=np.uint64)
    _lib.check(L.oem_debug_cells_records_last_csr(None, rp.ctypes.data, tid.ctypes.data, p.ctypes.data, s.ctypes.data,
                                                  e.ctypes.data, cro.ctypes.data))
    return rp, tid, p, s, e, cro


def test_the_device_csr_is_the_builders_byte_for_byte(small_cells, monkeypatch):
    fx = small_cells
    monkeypatch.setenv(KEEP, "1")
    with _lib.testing() as L:
        _run(fx["filters"], fx["txp_len"], fx["pieces"], max_iter=5)
        assert len(_last_paths()) == 1          # one group holds every cell
        rp, tid, p, s, e, cro = _kept_csr(L)
    host = fx["host"]
    want_rp, want_cro, base = [np.zeros(1, dtype=np.uint64)], [0], 0
    for h in host:
        want_rp.append(h["rp"][1:] + np.uint64(base))
        base += len(h["tid"])
        want_cro.append(want_cro[-1] + len(h["rp"]) - 1)
    assert np.array_equal(rp.astype(np.uint64), np.concatenate(want_rp))
    assert np.array_equal(cro, np.array(want_cro, dtype=np.uint64))
    assert tid.tobytes() == np.concatenate([h["tid"] for h in host]).tobytes()
    assert p.tobytes() == np.concatenate([h["p"] for h in host]).tobytes()       # as_prob, bit for bit
    assert s.tobytes() == np.concatenate([h["s"] for h in host]).tobytes()
    assert e.tobytes() == np.concatenate([h["e"] for h in host]).tobytes()


# ---- fixture 3: cells of 300 to 2 000 reads ----------------------------------------------------------------------------
READS = [300, 2000, 700, 1200, 450, 1600, 900, 350, 1900, 600, 1000, 1400]
NO_GROUPS, ALL_DROPPED = 4, 9     # where the two spliced cells end up


def _dropped_cell():
    """15 reads that the filter drops: unmapped records only, a non-positive best score, a short best alignment."""
    rec = np.zeros(20, dtype=ALN_RECORD)
    rec["seq_len"] = -1
    goff = [0]
    i = 0
    for k in range(15):
        if k % 3 == 0:
            rec["ref_id"][i:i + 2] = 0xFFFFFFFF
            rec["flags"][i:i + 2] = _lib.REC_UNMAPPED
            i += 2
        else:
            rec[i] = (k, 0, 390, 100, 0 if k % 3 == 1 else 1000, 100 if k % 3 == 1 else 1000, _lib.REC_HAS_SCORE, 0)
            i += 1
        goff.append(i)
    return rec[:i].copy(), np.array(goff, dtype=np.uint64)


@pytest.fixture(scope="module")
def cells():
    return _cells()


def _cells():
    stores = [synth.make_cells(1, r, T, kbar=4.0, seed=201 + k, expressed_frac=0.1 if k % 2 else None) for k, r in enumerate(READS)]
    co, rps, tids, ps, base = [0], [np.zeros(1, dtype=np.uint64)], [], [], 0
    for _, rp, tid, p in stores:
        rps.append(rp[1:] + np.uint64(base))
        tids.append(tid)
        ps.append(p)
        base += len(tid)
        co.append(co[-1] + len(rp) - 1)
    cr = synth.make_cell_records((np.array(co, dtype=np.uint64), np.concatenate(rps), np.concatenate(tids), np.concatenate(ps)),
                                 T, seed=7)
    pieces = _split(cr.records, cr.group_off, cr.cell_group_off)
    pieces.insert(NO_GROUPS, (np.zeros(0, dtype=ALN_RECORD), np.zeros(1, dtype=np.uint64)))
    pieces.insert(ALL_DROPPED, _dropped_cell())
    host = _host_way(cr.filters, cr.txp_len, pieces)
    assert len(host[NO_GROUPS]["kept"]) == 0
    assert len(host[ALL_DROPPED]["kept"]) == 15 and not host[ALL_DROPPED]["kept"].any()
    n_groups = sum(len(h["kept"]) for h in host)
    n_kept = sum(int((h["kept"] > 0).sum()) for h in host)
    assert n_kept >= 0.9 * n_groups and n_groups - n_kept >= 10, (n_groups, n_kept)
    fx = dict(filters=cr.filters, txp_len=cr.txp_len, pieces=pieces, host=host, want={})
    return fx


def _want(fx, model):
    if model not in fx["want"]:
        fx["want"][model] = _oracle(fx["host"], fx["txp_len"], T, model)
        niters = [wi.niter for _, wi in fx["want"][model]]
        assert min(niters) < MAX_ITER, niters
    return fx["want"][model]


@pytest.mark.parametrize("model", [-1, 0, 1])
def test_every_cell_matches_the_oracle(cells, model):
    got = _run(cells["filters"], cells["txp_len"], cells["pieces"], model)
    _check_filter_side(got, cells["host"], f"model {model}")
    _check_em_side(got, cells["host"], _want(cells, model), T, f"model {model}")
    indptr, infos = got[0], got[3]
    for c in (NO_GROUPS, ALL_DROPPED):     # no entries, and the info of a cell without reads
        assert indptr[c] == indptr[c + 1] and repr(infos[c]) == repr(infos[NO_GROUPS])


@pytest.mark.parametrize("host_layout", [False, True])
@pytest.mark.parametrize("model", [-1, 1])
def test_group_cuts_and_the_cell_that_exceeds_the_bound(cells, model, host_layout, monkeypatch):
    n_rec = np.array([len(r) for r, _ in cells["pieces"]])
    big = int(n_rec.argmax())
    monkeypatch.setenv("OEM_CELLS_GROUP_NNZ", str(int(n_rec.max()) - 1))       # (the bound counts records here)
    if host_layout:
        monkeypatch.setenv("OEM_TEST_HOST_LAYOUT", "1")
    with _lib.testing():
        got = _run(cells["filters"], cells["txp_len"], cells["pieces"], model)
        paths = _last_paths()
    assert len(paths) >= 3 and (big, big + 1, 0) in paths, paths      # the cell alone: cell by cell
    assert sum(1 for _, _, b in paths if b) >= 2, paths
    assert paths[0][0] == 0 and paths[-1][1] == len(n_rec) and all(a[1] == b[0] for a, b in zip(paths, paths[1:]))
    label = f"groups, model {model}, host layout {host_layout}"
    _check_filter_side(got, cells["host"], label)
    _check_em_side(got, cells["host"], _want(cells, model), T, label)


@pytest.mark.parametrize("case", ["big_score", "inf_denom"])
def test_host_loop_fallbacks(cells, case):
    """A mapped score beyond 2^24 (found by the measure pass) and a score_prob_denom without a gap table: the group takes
    the host loop, with the result of the long way round."""
    pieces = [(r.copy(), g) for r, g in cells["pieces"][:6]]
    filters = dict(cells["filters"])
    if case == "big_score":
        rec = pieces[2][0]
        i = int(np.flatnonzero((rec["flags"] & _lib.REC_UNMAPPED) == 0)[5])
        rec["score"][i] = 2 ** 24 + 1
        rec["flags"][i] |= _lib.REC_HAS_SCORE
    else:
        filters["score_prob_denom"] = float("inf")
    host = _host_way(filters, cells["txp_len"], pieces)
    got = _run(filters, cells["txp_len"], pieces)
    _check_filter_side(got, host, case)
    _check_em_side(got, host, _oracle(host, cells["txp_len"], T, -1), T, case)
    if case == "inf_denom":
        assert all(np.all(h["p"] == 1.0) for h in host)


def test_edge_groups_one_cell_each():
    by_filters = {}
    for name, F, txp_len, group in fc.edge_groups():
        by_filters.setdefault((tuple(sorted(fc.filters_dict(F).items())), tuple(txp_len)), []).append((name, group))
    assert len(by_filters) >= 5
    for (fkey, txp_len), named in by_filters.items():
        filters = dict(fkey)
        pieces = [fc.pack([g]) for _, g in named]
        host = _host_way(filters, np.array(txp_len, dtype=np.uint64), pieces)
        got = _run(filters, np.array(txp_len, dtype=np.uint64), pieces, max_iter=3)
        _check_filter_side(got, host, "edge groups: " + ", ".join(n for n, _ in named))


def test_device_errors_name_the_cell(cells):
    pieces = [(r.copy(), g) for r, g in cells["pieces"][:5]]
    rec = pieces[2][0]
    i = int(np.flatnonzero((rec["flags"] & _lib.REC_UNMAPPED) == 0)[40])
    rec["ref_id"][i] = T
    where = sum(len(r) for r, _ in pieces[:2]) + i
    with pytest.raises(oarfish_amd.OemError) as ei:
        _run(cells["filters"], cells["txp_len"], pieces)
    assert ei.value.code == _lib.OEM_ERR_ARG and "cell 2" in str(ei.value) and f"record {where}:" in str(ei.value), str(ei.value)
    L = _lib.lib()      # ... and *out is NULL
    r, goff, cgo = _concat(pieces)
    from oarfish_amd.builder import filters_c
    F = filters_c(cells["filters"])
    res = C.c_void_p(1)
    rc = L.oem_em_run_cells_records_sparse(C.addressof(F), cells["txp_len"].ctypes.data, T, r.ctypes.data, goff.ctypes.data,
                                           len(goff) - 1, cgo.ctypes.data, len(cgo) - 1, 0, -1, 0.0, 0, MAX_ITER, 1e-3, None,
                                           C.byref(res))
    assert rc == _lib.OEM_ERR_ARG and not res.value

    pieces = [(r.copy(), g) for r, g in cells["pieces"][:5]]
    host = cells["host"][3]
    rec, goff = pieces[3]
    g = int(np.flatnonzero(host["kept"] > 0)[7])                # read 7 of the cell's store: its first alignment, past the end
    a = int(host["rp"][7])
    same = [j for j in range(int(goff[g]), int(goff[g + 1]))
            if (int(rec["ref_id"][j]), int(rec["aln_start"][j]), int(rec["aln_end"][j])) == (int(host["tid"][a]), int(host["s"][a]), int(host["e"][a]))]
    assert len(same) == 1
    j = same[0]
    rec["aln_end"][j] = 2 * int(cells["txp_len"][rec["ref_id"][j]])     # (add_interval: past the bin after the last one)
    assert _host_way(cells["filters"], cells["txp_len"], [pieces[3]])[0]["kept"][g] == host["kept"][g]
    with pytest.raises(oarfish_amd.OemError) as ei:
        _run(cells["filters"], cells["txp_len"], pieces, model=1)
    assert ei.value.code == _lib.OEM_ERR_STATE and "cell 3" in str(ei.value) and "outside its transcript" in str(ei.value)


# ---- the records session ---------------------------------------------------------------------------------------------
def _push_all(cs, pieces, n_threads=4, seed=7):
    """Every cell, in a shuffled order, from n_threads threads (the shape of tests/test_cells_stream_gpu.py's)."""
    n = len(pieces)
    order = np.random.default_rng(seed).permutation(n)
    cell_of_ticket, errors = {}, []
    lock = threading.Lock()

    def work(k):
        try:
            for c in order[k::n_threads]:
                t = cs.push_records(*pieces[int(c)])
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


@pytest.mark.parametrize("model", [-1, 1])
def test_a_records_session_from_four_threads(cells, model):
    cov = None if model < 0 else dict(COVS[model], txp_len=cells["txp_len"])
    with oarfish_amd.CellsStream(T, max_iter=MAX_ITER, conv_thresh=1e-3, coverage=cov, filters=cells["filters"],
                                 txp_len=cells["txp_len"], group_cells=5) as cs:
        tickets = _push_all(cs, cells["pieces"])
        got = cs.finish()
        tables = cs.discard_tables()
        info = cs.info()
    n = len(tickets)
    assert info["cells"] == n and info["groups"] >= 3 and info["alignments"] == sum(len(r) for r, _ in cells["pieces"])
    host = [cells["host"][tickets[k]] for k in range(n)]
    want = [_want(cells, model)[tickets[k]] for k in range(n)]
    _check_em_side(got, host, want, T, f"records session, model {model}")
    assert [tables[k] for k in range(n)] == [h["table"] for h in host]


def test_session_state_errors(cells):
    pieces = cells["pieces"]
    h0 = cells["host"][0]
    with oarfish_amd.CellsStream(T, max_iter=MAX_ITER, filters=cells["filters"], txp_len=cells["txp_len"]) as cs:
        with pytest.raises(oarfish_amd.OemError) as ei:     # push on a records session
            cs.push(h0["rp"], h0["tid"], h0["p"])
        assert ei.value.code == _lib.OEM_ERR_STATE
        rec, goff = pieces[0]
        bad = goff.copy()
        bad[3], bad[4] = goff[4], goff[3] - 1
        assert bad[4] < bad[3]
        with pytest.raises(oarfish_amd.OemError) as ei:     # a malformed group_off rejects that cell only
            cs.push_records(rec, bad)
        assert ei.value.code == _lib.OEM_ERR_ARG and "group_off decreases" in str(ei.value)
        assert cs.push_records(rec, goff) == 0              # ... and uses no ticket
        with pytest.raises(oarfish_amd.OemError) as ei:     # set_filters after a push
            cs.set_filters(cells["filters"], cells["txp_len"])
        assert ei.value.code == _lib.OEM_ERR_STATE
        assert cs.push_records(*pieces[2]) == 1
        got = cs.finish()
        tables = cs.discard_tables()
        with pytest.raises(oarfish_amd.OemError) as ei:     # ... and after finish
            cs.set_filters(cells["filters"], cells["txp_len"])
        assert ei.value.code == _lib.OEM_ERR_STATE
    host = [cells["host"][0], cells["host"][2]]
    _check_em_side(got, host, [_want(cells, -1)[0], _want(cells, -1)[2]], T, "records session, two cells")
    assert tables == [h["table"] for h in host]
    with oarfish_amd.CellsStream(T, max_iter=MAX_ITER) as cs:       # push_records on a plain session
        with pytest.raises(oarfish_amd.OemError) as ei:
            cs.push_records(*pieces[0])
        assert ei.value.code == _lib.OEM_ERR_STATE
        assert cs.push(h0["rp"], h0["tid"], h0["p"]) == 0
        cs.finish()
        with pytest.raises(oarfish_amd.OemError) as ei:             # a plain session's result has no tables
            cs.discard_tables()
        assert ei.value.code == _lib.OEM_ERR_STATE
    with oarfish_amd.CellsStream(T, max_iter=MAX_ITER, filters=cells["filters"], txp_len=cells["txp_len"]) as cs:
        indptr, cols, vals, infos = cs.finish()                     # a session without cells
        assert list(indptr) == [0] and len(cols) == 0 and len(vals) == 0 and infos == [] and cs.discard_tables() == []


def test_a_ref_id_error_in_a_session_is_sticky_and_names_the_ticket(cells):
    pieces = [(r.copy(), g) for r, g in cells["pieces"][:3]]
    rec = pieces[1][0]
    i = int(np.flatnonzero((rec["flags"] & _lib.REC_UNMAPPED) == 0)[3])
    rec["ref_id"][i] = T + 5
    with oarfish_amd.CellsStream(T, max_iter=MAX_ITER, filters=cells["filters"], txp_len=cells["txp_len"]) as cs:
        for p in pieces:
            cs.push_records(*p)
        with pytest.raises(oarfish_amd.OemError) as ei:
            cs.finish()
        assert ei.value.code == _lib.OEM_ERR_ARG and "cell 1" in str(ei.value) and "n_txps" in str(ei.value), str(ei.value)
