"""GPU tests of every path of the per-cell driver (oem_cells.hip: run_cells / run_cells_group / run_cells_batched)
through each of its three sinks -- dense (oem_em_run_cells), sparse (oem_em_run_cells_sparse) and fused coverage + EM
(oem_em_run_cells_coverage_sparse) -- against the oracle's em::em on every cell's own store (single_cell.rs:139-160),
not against another call that shares the path.  The test-only library records the groups of the last call and the
path each one took (oem_debug_cells_last_paths), which proves that a case reaches the path it is named after."""
import ctypes as C

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth
from oracle import c_oracle
from oracle import filter_py as fp
from tests.common import assert_cell_matches_oracle
from tests.test_cells_coverage_gpu import _assert_close, _join
from tests.test_cells_sparse_gpu import _check_structure

pytestmark = pytest.mark.gpu

T = 600
MAX_ITER = 60          # with em::em's gate of 50: some cells converge, the others stop at max_iter, in one call
HEAD = 6               # the forced head split: the head ends with an empty cell (HEAD - 1)
DECLINE = 16           # the declining cell of the second fixture
SPLIT = {"OEM_CELLS_SPLIT_NNZ": "0", "OEM_CELLS_SPLIT_CELLS": "2"}   # (the product splits >= 64 cells, >= 64 Mi aln)
COV = dict(bin_width=100, model="binomial", growth_rate=2.0)


# ---- the cells -----------------------------------------------------------------------------------------------------
def _gen_cells(n, reads, seed, expressed_frac):
    co, rp, tid, p = synth.make_cells(n, reads, T, kbar=4.0, seed=seed, expressed_frac=expressed_frac)
    out = []
    for c in range(n):
        r0, r1 = int(co[c]), int(co[c + 1])
        a0, a1 = int(rp[r0]), int(rp[r1])
        out.append((rp[r0:r1 + 1] - rp[r0], tid[a0:a1], p[a0:a1]))
    return out


def _single_reads(tids, rng):
    """A cell of reads with one alignment each."""
    tids = np.asarray(tids, np.uint32)
    return np.arange(len(tids) + 1, dtype=np.uint64), tids, rng.uniform(0.1, 1.0, len(tids)).astype(np.float32)


def _decline_cell(rng):
    """A read with 300 alignments inside one tile window, as in the bulk store's test: the tiler declines the batch."""
    lens = np.concatenate([[300], rng.integers(1, 9, size=1_500)])
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    tid = np.concatenate([np.arange(100, 400), (np.repeat(rng.integers(0, T, size=1_500), lens[1:]) +
                                                rng.integers(0, 5, size=int(lens[1:].sum()))) % T]).astype(np.uint32)
    return rp, tid, np.exp(-rng.integers(0, 30, size=len(tid)) / 5.0).astype(np.float32)


def _cells(decline):
    """~20 cells over 600 transcripts.  Generated cells of 2 000 reads, half over a tenth of the annotation (they
    converge within 60 iterations) and half over all of it (they run into max_iter), and the edges:
    empty cells first, last, on either side of a forced head split and at the end of a group; a head of empty cells
    only (cells 0 and 1); a one-read cell and a one-alignment cell; a cell all on transcript T - 1 and one all on
    transcript 0; a cell of unique reads only; a cell whose reads repeat a transcript; a cell whose every read has a
    zero-span alignment (all dropped).  `decline`: one more cell, with a read the tiler cannot take."""
    rng = np.random.default_rng(0xCE11)
    conv = _gen_cells(6, 2_000, 101, 0.1)
    full = _gen_cells(4, 2_000, 103, None)
    empty = (np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32))
    rep_rp, rep_tid, rep_p = _gen_cells(1, 300, 107, 0.05)[0]
    lens = np.diff(rep_rp.astype(np.int64))
    first = rep_rp[:-1].astype(np.int64)
    multi = lens >= 2
    rep_tid = rep_tid.copy()
    rep_tid[first[multi] + 1] = rep_tid[first[multi]]          # every multi-mapping read names a transcript twice
    cells = [
        empty, empty,                                                         # 0, 1: a head of empty cells
        conv[0],                                                              # 2
        (np.array([0, 5], np.uint64), np.array([10, 50, 51, 200, T - 1], np.uint32),
         np.array([0.9, 0.5, 0.5, 0.2, 0.1], np.float32)),                   # 3: one read
        (np.array([0, 1], np.uint64), np.array([7], np.uint32), np.array([0.8], np.float32)),   # 4: one alignment
        empty,                                                                # 5 = HEAD - 1
        full[0],                                                              # 6 = HEAD
        _single_reads(np.full(30, T - 1), rng),                               # 7: all on T - 1
        conv[1],                                                              # 8
        _single_reads(rng.integers(0, T, 400), rng),                          # 9: unique reads only
        (rep_rp, rep_tid, rep_p),                                             # 10: reads that repeat a transcript
        full[1],                                                              # 11
        _gen_cells(1, 200, 109, None)[0],                                     # 12: every read dropped
        conv[2],                                                              # 13
        empty,                                                                # 14: the end of a group
        full[2],                                                              # 15
        _single_reads(np.zeros(25), rng),                                     # 16: all on transcript 0
        conv[3], conv[4], full[3], conv[5],                                   # 17 .. 20
        empty,                                                                # 21: the last cell
    ]
    if decline:
        cells.insert(DECLINE, _decline_cell(rng))       # (with the small cell after it: a group of two)
    cell_off, row_ptr, tid = _join([(rp, t) for rp, t, _ in cells])
    p = np.concatenate([q for _, _, q in cells]).astype(np.float32)
    tl, s, e = synth.make_coordinates(tid, T, seed=113)
    assert np.all(e > s)
    dropped = 12
    r0, r1 = int(cell_off[dropped]), int(cell_off[dropped + 1])
    e[row_ptr[r0:r1].astype(np.int64)] = s[row_ptr[r0:r1].astype(np.int64)]   # a zero-span alignment in every read
    rest = np.setdiff1d(np.arange(len(tid)), np.arange(int(row_ptr[r0]), int(row_ptr[r1])))
    z = rng.choice(rest, 40, replace=False)                                    # and a few reads dropped elsewhere
    e[z] = s[z]
    return dict(cell_off=cell_off, row_ptr=row_ptr, tid=tid, p=p, s=s, e=e, tl=tl, dropped=dropped)


def _cell(fx, c):
    r0, r1 = int(fx["cell_off"][c]), int(fx["cell_off"][c + 1])
    return r0, r1, int(fx["row_ptr"][r0]), int(fx["row_ptr"][r1])


def _with_oracle(fx):
    """The per-cell reference, once per fixture: filter_py.coverage_probs on each cell's own store (NaN at a zero-span
    alignment), and em::em (gate 50, init None, the cell's own read count) on that column for MAX_ITER and for 0
    iterations.  Dense and sparse take the same column as their coverage input, so one answer serves all three sinks."""
    cov = np.zeros(len(fx["tid"]))
    want = {MAX_ITER: [], 0: []}
    for c in range(len(fx["cell_off"]) - 1):
        r0, r1, a0, a1 = _cell(fx, c)
        rp = fx["row_ptr"][r0:r1 + 1] - fx["row_ptr"][r0]
        st = fp.Store(row_ptr=[int(x) for x in rp], tid=[int(x) for x in fx["tid"][a0:a1]],
                      start=[int(x) for x in fx["s"][a0:a1]], end=[int(x) for x in fx["e"][a0:a1]])
        cov[a0:a1] = fp.coverage_probs(st, [int(x) for x in fx["tl"]], COV["bin_width"], COV["growth_rate"],
                                       model=COV["model"])
        o = c_oracle.Store(rp, fx["tid"][a0:a1], fx["p"][a0:a1], cov[a0:a1], T)
        for mi in want:
            want[mi].append(c_oracle.do_em(o, max_iter=mi, conv_thresh=1e-3, min_iter_gate=50))
    r0, r1, a0, a1 = _cell(fx, fx["dropped"])
    assert np.all(np.isnan(np.add.reduceat(cov[a0:a1], (fx["row_ptr"][r0:r1] - a0).astype(np.int64))))
    assert not np.any(want[MAX_ITER][fx["dropped"]][0])
    niters = [wi.niter for _, wi in want[MAX_ITER]]
    assert min(niters) < MAX_ITER and max(niters) == MAX_ITER, niters
    fx.update(cov=cov, want=want)
    return fx


@pytest.fixture(scope="module")
def plain():
    return _with_oracle(_cells(decline=False))


@pytest.fixture(scope="module")
def declining():
    return _with_oracle(_cells(decline=True))


# ---- the driver's grouping rule (oem_cells.hip run_cells), for OEM_CELLS_GROUP_NNZ ----------------------------------
def _group_nnz(fx):
    """A group bound that keeps one generated cell per group: the small and empty cells after it join its group."""
    nnz = np.diff(fx["row_ptr"][fx["cell_off"].astype(np.int64)].astype(np.int64))
    return int(nnz.max())


def _groups(fx, limit):
    nnz = np.diff(fx["row_ptr"][fx["cell_off"].astype(np.int64)].astype(np.int64))
    n = len(nnz)
    out, c0 = [], 0
    while c0 < n:
        c1 = c0 + 1
        while c1 < n and nnz[c0:c1 + 1].sum() <= limit:
            c1 += 1
        out.append((c0, c1))
        c0 = c1
    return out


def _last_paths():
    n = C.c_uint32()
    buf = (C.c_uint32 * (3 * 64))()
    _lib.check(_lib.testing_lib().oem_debug_cells_last_paths(C.byref(n), C.addressof(buf), 64))
    assert n.value <= 64
    return [(buf[3 * g], buf[3 * g + 1], buf[3 * g + 2]) for g in range(n.value)]


# ---- one call through one sink -------------------------------------------------------------------------------------
def _subset(fx, cells):
    """The fixture restricted to consecutive cells [c0, c1) (row_ptr rebased), with their oracle answers."""
    c0, c1 = cells
    r0, r1 = int(fx["cell_off"][c0]), int(fx["cell_off"][c1])
    a0, a1 = int(fx["row_ptr"][r0]), int(fx["row_ptr"][r1])
    sub = dict(fx)
    sub["cell_off"] = fx["cell_off"][c0:c1 + 1] - fx["cell_off"][c0]
    sub["row_ptr"] = fx["row_ptr"][r0:r1 + 1] - fx["row_ptr"][r0]
    for k in ("tid", "p", "s", "e", "cov"):
        sub[k] = fx[k][a0:a1]
    sub["want"] = {mi: w[c0:c1] for mi, w in fx["want"].items()}
    return sub


def _run(sink, fx, max_iter):
    a = (fx["cell_off"], fx["row_ptr"], fx["tid"], fx["p"])
    if sink == "dense":
        return oarfish_amd.em_cells(*a, fx["cov"], T, max_iter=max_iter, convergence_thresh=1e-3)
    if sink == "sparse":
        return oarfish_amd.em_cells_sparse(*a, fx["cov"], T, max_iter=max_iter, convergence_thresh=1e-3)
    return oarfish_amd.em_cells_coverage_sparse(*a, fx["s"], fx["e"], fx["tl"], **COV, max_iter=max_iter,
                                                convergence_thresh=1e-3, return_coverage=True)


def _check(sink, got, fx, max_iter, label):
    """Every cell against the oracle; the fused call's column against filter_py's, NaN in the same places."""
    cell_off = fx["cell_off"]
    n = len(cell_off) - 1
    want = fx["want"][max_iter]
    reads = np.diff(cell_off.astype(np.int64))
    if sink == "dense":
        out, infos = got
        assert out.shape == (n, T) and len(infos) == n, label
        for c in range(n):
            assert_cell_matches_oracle(infos[c], want[c], int(reads[c]), T, f"{label}: cell {c}", dense=out[c])
        return
    indptr, cols, vals, infos = got[:4]
    _check_structure(indptr, cols, vals, n, T)
    assert len(infos) == n, label
    for c in range(n):
        s = slice(int(indptr[c]), int(indptr[c + 1]))
        assert_cell_matches_oracle(infos[c], want[c], int(reads[c]), T, f"{label}: cell {c}", cols=cols[s], vals=vals[s])
    if sink == "fused" and len(fx["cov"]):
        _assert_close(got[4], fx["cov"], 1e-9, f"{label}: coverage column")


# ---- the paths -----------------------------------------------------------------------------------------------------
SINKS = ["dense", "sparse", "fused"]


def _case(path, fx, monkeypatch):
    """(fixture, max_iter, the groups [(c0, c1, 1 if batched else 0)] the call must report) of a path; sets its knobs."""
    n = len(fx["cell_off"]) - 1
    knobs, max_iter, groups = {}, MAX_ITER, [(0, n, 1)]
    if path == "serial":
        knobs["OEM_SERIAL_CELLS"] = "1"
        groups = [(0, n, 0)]
    elif path.startswith("groups_w"):
        limit = _group_nnz(fx)
        knobs.update(OEM_CELLS_GROUP_NNZ=str(limit), OEM_CELLS_WORKERS=path[-1])
        groups = [(c0, c1, int(c1 - c0 >= 2)) for c0, c1 in _groups(fx, limit)]
        assert len(groups) >= 6 and any(c1 == 15 for _, c1, _ in groups)   # empty cell 14 ends a group
    elif path == "head_split":
        knobs.update(SPLIT, OEM_CELLS_HEAD=str(HEAD))
        groups = [(0, HEAD, 1), (HEAD, n, 1)]
    elif path == "tail_starts_empty":
        knobs.update(SPLIT, OEM_CELLS_HEAD=str(HEAD - 1))
        groups = [(0, HEAD - 1, 1), (HEAD - 1, n, 1)]
    elif path == "empty_head":        # a group without alignments cannot be tiled: it runs cell by cell
        knobs.update(SPLIT, OEM_CELLS_HEAD="2")
        groups = [(0, 2, 0), (2, n, 1)]
    elif path == "uncompacted":
        knobs["OEM_TEST_FAIL_RANK_ALLOC"] = "1"
    elif path == "full_alloc":
        knobs["OEM_TEST_FAIL_FULL_ALLOC"] = "1"
    elif path == "compact_txps_0":
        knobs["OEM_CELLS_COMPACT_TXPS"] = "0"
    elif path == "compact_0":
        knobs["OEM_CELLS_COMPACT"] = "0"
    elif path == "fused_fold_0":
        knobs["OEM_CELLS_FUSED_FOLD"] = "0"
    elif path == "host_layout":
        knobs["OEM_TEST_HOST_LAYOUT"] = "1"
    elif path == "cov_chunks":        # a bin budget of about two cells: the coverage of a group runs in sub-chunks
        knobs["OEM_COV_CELLS_CHUNK_BINS"] = "30000"
    elif path == "cov_chunks_split":
        knobs.update(SPLIT, OEM_CELLS_HEAD=str(HEAD), OEM_COV_CELLS_CHUNK_BINS="30000")
        groups = [(0, HEAD, 1), (HEAD, n, 1)]
    elif path == "max_iter_0":
        max_iter = 0
        groups = [(0, n, 0)]
    elif path == "one_cell":
        fx = _subset(fx, (2, 3))
        groups = [(0, 1, 0)]
    elif path == "no_cells":
        fx = _subset(fx, (0, 0))
        groups = []
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    return fx, max_iter, groups


PATHS = ["batched", "serial", "groups_w1", "groups_w2", "groups_w3", "groups_w4", "head_split", "tail_starts_empty",
         "empty_head", "uncompacted", "full_alloc", "compact_txps_0", "compact_0", "fused_fold_0", "host_layout",
         "cov_chunks", "cov_chunks_split", "max_iter_0", "one_cell", "no_cells"]
ONLY = {"full_alloc": ("dense",), "cov_chunks": ("fused",), "cov_chunks_split": ("fused",)}   # paths of one sink


@pytest.mark.parametrize("sink,path", [(k, p) for p in PATHS for k in ONLY.get(p, SINKS)])
def test_every_path_matches_the_oracle(sink, path, plain, monkeypatch):
    fx, max_iter, groups = _case(path, plain, monkeypatch)
    with _lib.testing():
        got = _run(sink, fx, max_iter)
        paths = _last_paths()
    assert paths == groups, (path, paths, groups)
    _check(sink, got, fx, max_iter, f"{sink}/{path}")
    if path == "batched":   # ... and the product library, whose knobs are fixed at their defaults
        _check(sink, _run(sink, fx, max_iter), fx, max_iter, f"{sink}/{path} (product)")


@pytest.mark.parametrize("where", ["one_group", "among_groups"])
@pytest.mark.parametrize("sink", SINKS)
def test_a_declined_group_matches_the_oracle(sink, where, declining, monkeypatch):
    """A group the tiler declines runs cell by cell (for the fused sink over the resident CSR the store hands back,
    with the caller's transcript ids restored); in a call of several groups only that group does."""
    fx = declining
    n = len(fx["cell_off"]) - 1
    dc = DECLINE
    r0, r1, _, _ = _cell(fx, dc)
    assert int(fx["row_ptr"][r0 + 1] - fx["row_ptr"][r0]) == 300
    if where == "one_group":
        groups = [(0, n, 0)]
    else:
        limit = _group_nnz(fx)
        monkeypatch.setenv("OEM_CELLS_GROUP_NNZ", str(limit))
        groups = [(c0, c1, int(c1 - c0 >= 2 and not c0 <= dc < c1)) for c0, c1 in _groups(fx, limit)]
        assert sum(1 for c0, c1, b in groups if b) >= 4 and sum(1 for c0, c1, b in groups if c1 - c0 >= 2 and not b) == 1
    with _lib.testing():
        got = _run(sink, fx, MAX_ITER)
        paths = _last_paths()
    assert paths == groups, (where, paths, groups)
    _check(sink, got, fx, MAX_ITER, f"{sink}/decline {where}")
