"""GPU tests of every reachable instantiation of the tile kernels, at shapes of a few tens of thousands of reads.

An E/M pass is served by one of a family of template instantiations, each a code object of its own with its own
register budget, pinning fences and hand-placed waits: k_em_tile<weight type, coding, window, record form, kNT>
(launch_em_pass_tiled, oem_tile_kernels.hip), k_em_tile_e<weight type / fused, record form, kNT> (launch_batch_pass,
oem_batch_kernels.hip) and k_remote_fold<kNTQ>.  The launchers choose by the store: its weights, its window cap,
whether its transcripts fit the packed record, and its SIZE -- a store streams non-temporally (kNT) above 192 MiB and
folds through the caches (kNTQ = false) above 96 MiB, which only the 10 M-read tests reach, on one store shape.  Here
the test-only library's OEM_TILE_NT / OEM_FOLD_NT choose instead, so every instantiation runs on the small stores
whose shapes make the kernels' distinct paths live (tests/common.tile_test_store), against the f64 oracle:

  long      reads with more than 16 local alignments: the reload loops behind the register sets
  remote    more remote records than a thread's six register slots; several fold workgroups per bucket
  ragged    a short last tile, single-alignment reads
  unpacked  2^22 + 12 345 transcripts: the packed record's transcript field overflows (the other record form)

Nothing is asserted on an assumption of what ran: after every step the case reads oem_debug_last_launch -- the
launchers' own record of the template arguments they launched with -- and holds it to the expected tuple; a combination
the layout cannot produce (a wide window never carries the fused or the 16-bit coding) names the variant the store
must fall to.  The last test holds the set of variants the module ran to the reachable set written down from the
dispatch code, so an instantiation cannot be added without a case.

The knobs exist in the test-only library alone.  The PRODUCT library's kNT code objects stay reachable through size
only: the full-size tests of tests/test_gpu_parity.py (test_full_size_c3_*, test_c5_slice_*) remain their check, and
the two builds of the tile sources differ by the OEM_TILE_EXP probe branches only.

Tolerances are the project's own (test_weight_dict_gpu.py, test_gpu_parity.py): one pass against
c_oracle.m_step 1e-10; a run of a fixed number of iterations against c_oracle.do_em (conv_thresh 0, equal niter
asserted) 1e-9; mass |sum - R| < 1e-7 R; the cached and the non-temporal pass over one store against each other 1e-12
(two orders of the same f64 sums: the atomics' order differs, nothing else)."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth
from oarfish_amd.types import DeviceStore
from oracle import c_oracle
from tests.common import assert_cell_matches_oracle, assert_counts_close, tile_test_store

pytestmark = pytest.mark.gpu

PLAIN, BYTES, FUSED, WORDS = 0, 1, 2, 3     # kWPlain, kWBytes, kWFused, kWWords (oem_tile_common.h)
N_ITER = 40                                 # below every gate: a run with conv_thresh 0 makes exactly 40 iterations
N_REP = 5                                   # more replicates than the four slots of the ONE chain the cases run
                                            # (OEM_BOOT_CHAINS=1): the slot that finishes first is handed the fifth

STORES = ["long", "remote", "ragged", "unpacked"]
VARIANTS = ["fused", "bytes", "words", "plain", "f64"]
WINDOWS = ["narrow", "wide"]

# What launch_em_pass_tiled must take for (weight variant, window): (f64 weights, coding).  Narrow: the coding the
# weights ask for.  Wide (oem_layout_dict.hip): at most 256 distinct weights are coded, as bytes -- never fused, never
# 16-bit -- so the generator's few dozen values fall to bytes and 600 values to the f32 stream.  f64 is always plain.
TILE = {
    ("fused", "narrow"): (0, FUSED), ("bytes", "narrow"): (0, BYTES), ("words", "narrow"): (0, WORDS),
    ("plain", "narrow"): (0, PLAIN), ("f64", "narrow"): (1, PLAIN),
    ("fused", "wide"): (0, BYTES), ("bytes", "wide"): (0, BYTES), ("words", "wide"): (0, PLAIN),
    ("plain", "wide"): (0, PLAIN), ("f64", "wide"): (1, PLAIN),
}
# ... and launch_batch_pass: (f64 weights, fused).  Only the fused coding has a batched kernel of its own; byte- and
# word-coded stores read their f32 stream there.  A wide store does not batch at all (can_batch): its replicates run
# one per pass through k_em_tile.
BATCH = {"fused": (0, 1), "bytes": (0, 0), "words": (0, 0), "plain": (0, 0), "f64": (1, 0)}

# the reachable sets, from the dispatch code: (wide, f64, coding, packed, nt) / (f64, fused, packed, nt) / ntq
REACHABLE_TILE = {(w, f, c, pk, nt)
                  for w, fc in ((0, [(0, PLAIN), (0, BYTES), (0, FUSED), (0, WORDS), (1, PLAIN)]),
                                (1, [(0, PLAIN), (0, BYTES), (1, PLAIN)]))
                  for f, c in fc for pk in (0, 1) for nt in (0, 1)}
REACHABLE_BATCH = {(f, fu, pk, nt) for f, fu in ((0, 0), (0, 1), (1, 0)) for pk in (0, 1) for nt in (0, 1)}
REACHABLE_FOLD = {0, 1}
assert len(REACHABLE_TILE) == 32 and len(REACHABLE_BATCH) == 12

_SEEN = {"tile": set(), "batch": set(), "fold": set(), "cells": set()}
_RAN = set()    # the cases of the matrix and of the per-cell batch that ran in this process (the completeness test)


# ---- stores, weights, references (computed once, shared, never written to) ------------------------------------------
@functools.lru_cache(maxsize=None)
def _csr(store):
    if store == "unpacked":
        T = (1 << 22) + 12_345
        st = synth.make_store(60_000, T, seed=909)
        assert st.tid.max() >= (1 << 22)
        out = st.row_ptr, st.tid, st.as_prob, T
    else:
        out = tile_test_store(store, seed=23)
    for a in out[:3]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _weights(store, variant):
    """(as_prob, cov_prob, weight_coding) of a weight variant on the store's CSR."""
    _, tid, p, _ = _csr(store)
    rng = np.random.default_rng(77)
    if variant in ("fused", "plain"):       # the generator's weights: a few dozen distinct values
        assert len(np.unique(p)) < 128
        return p, None, 1 if variant == "plain" else 0
    if variant in ("bytes", "words"):
        n = 200 if variant == "bytes" else 600
        q = np.exp(-rng.integers(0, n, size=len(tid)) / 40.0).astype(np.float32)
        q[:n] = np.exp(-np.arange(n) / 40.0).astype(np.float32)
        assert len(np.unique(q)) == n
        return q, None, 0
    if variant == "f64":                    # a coverage column: f64 products
        return p, rng.uniform(1e-3, 1.0, size=len(tid)), 0
    raise ValueError(variant)


@functools.lru_cache(maxsize=None)
def _inputs(store):
    row_ptr, _, _, T = _csr(store)
    R = len(row_ptr) - 1
    rng = np.random.default_rng(5)
    theta = rng.lognormal(0.0, 1.5, T)
    theta[rng.random(T) < 0.1] = 0.0
    row_w = rng.poisson(1.0, size=R).astype(np.uint32)
    boot_w = rng.multinomial(R, np.full(R, 1.0 / R), size=N_REP).astype(np.uint32)
    assert boot_w.max() < 256
    return theta, row_w, boot_w


@functools.lru_cache(maxsize=2)             # (the cases of one (store, variant) follow each other)
def _reference(store, variant):
    row_ptr, tid, _, T = _csr(store)
    p, cov, _ = _weights(store, variant)
    theta, row_w, boot_w = _inputs(store)
    o = c_oracle.Store(row_ptr, tid, p, cov, T)
    em, info = c_oracle.do_em(o, max_iter=N_ITER, conv_thresh=0.0, min_iter_gate=50)
    assert info.niter == N_ITER
    boots = []
    for b in range(N_REP):
        cnt, bi = c_oracle.do_em(o, max_iter=N_ITER, conv_thresh=0.0, min_iter_gate=50, row_w=boot_w[b])
        assert bi.niter == N_ITER
        boots.append(cnt)
    return dict(m=c_oracle.m_step(o, theta), mw=c_oracle.m_step(o, theta, row_w=row_w), em=em, boots=boots)


def _open(store, variant, window):
    row_ptr, tid, _, T = _csr(store)
    p, cov, coding = _weights(store, variant)
    return DeviceStore(row_ptr, tid, p, cov, T, window_cap=2048 if window == "wide" else 512, weight_coding=coding)


# ---- the record ---------------------------------------------------------------------------------------------------------
def _last_launch(d=None):
    """(tile, batch, fold) the launchers recorded on `d` since the last look (None: that family launched nothing), or in
    the batched group of this thread's last per-cell call.  tile = (wide, f64, coding, packed, nt, per-cell batch),
    batch = (f64, fused, packed, nt), fold = (ntq, workgroups per bucket)."""
    out = (C.c_uint32 * 15)()
    _lib.check(_lib.lib().oem_debug_last_launch(d.handle if d is not None else None, out, 15))
    v = [int(x) for x in out]
    tile = tuple(v[1:7]) if v[0] else None
    batch = tuple(v[8:12]) if v[7] else None
    fold = tuple(v[13:15]) if v[12] else None
    if tile and not tile[5]:
        _SEEN["tile"].add(tile[:5])
    if tile and tile[5]:
        _SEEN["cells"].add(tile[:5])
    if batch:
        _SEEN["batch"].add(batch)
    if fold:
        _SEEN["fold"].add(fold[0])
    return tile, batch, fold


def _check_fold(got, ntq, has_remote, store, what):
    """A store with remote alignments folds with k_remote_fold<ntq>, in at least one workgroup per bucket; one without
    launches no fold.  The grid itself is tuning, not pinned here -- except that the mostly-remote store (some 45 k
    queue entries per bucket against the 8 Ki a workgroup is given) must fold with several, or the split of a bucket
    between workgroups would run nowhere."""
    if not has_remote:
        assert got is None, (what, got)
        return
    assert got is not None and got[0] == ntq and got[1] >= 1, (what, got)
    if store == "remote":
        assert got[1] > 1, (what, got)


def _set_nt(monkeypatch, nt):
    """One switch for the three launchers: nt = 1 runs the non-temporal form of the tile kernel, of the batched tile
    kernel and of the fold, nt = 0 the cached form of all three -- so a case with nt = 0 executes no non-temporal load
    of the streams at all, and a fault of the kNT bodies shows in the nt = 1 cases alone.  (By size the fold pairs the
    other way round: a small store folds non-temporally.  The default is held by its own test below.)  That holds with
    the compile-time switches OEM_REC_NT and OEM_E_MULT_NT at their default 0, and the first of them also means that
    the remote RECORDS are loaded through the caches in both halves: what kNT changes is the loads of the slices (and,
    in the fold, of the queue), so packed / unpacked x nt are four code objects that differ by their slice loads and
    their record decoding, not four ways of loading a record."""
    monkeypatch.setenv("OEM_TILE_NT", str(nt))
    monkeypatch.setenv("OEM_FOLD_NT", str(nt))


def _clear_knobs(monkeypatch):
    for k in ("OEM_TILE_NT", "OEM_FOLD_NT", "OEM_DICT_NO_FUSE", "OEM_NO_DICT", "OEM_WINDOW_CAP", "OEM_TILE_EXP",
              "OEM_BOOT_CHAINS"):
        monkeypatch.delenv(k, raising=False)


def _one_chain(monkeypatch):
    """The batched bootstrap starts two chains of four slots for more than four replicates, and their eight slots would
    take the five replicates at once.  One chain: four start, and the fifth goes to the slot that finishes first while
    the others run on."""
    monkeypatch.setenv("OEM_BOOT_CHAINS", "1")


def _run_case(d, ref, store, what, tile, batch, ntq, steps=("m", "mw", "em", "boot1", "boot0")):
    """The steps of a case on an open store: each against its reference, each with the record of what it launched."""
    row_ptr, _, _, T = _csr(store)
    R = len(row_ptr) - 1
    theta, row_w, boot_w = _inputs(store)
    fold = d.info(_lib.OEM_INFO_REMOTE_ALIGNMENTS) > 0
    _last_launch(d)   # (the record starts empty)

    def launched(step, want_tile, want_batch, want_fold):
        got = _last_launch(d)
        assert got[:2] == (want_tile, want_batch), (what, step, got)
        _check_fold(got[2], ntq, bool(want_fold), store, (what, step))

    if "m" in steps:
        m = d.m_step(theta)
        launched("m_step", tile, None, fold)
        assert_counts_close(m, ref["m"], R, T, 1e-10, f"{what}: m_step")
    if "mw" in steps:
        m = d.m_step(theta, row_w)
        launched("m_step with multiplicities", tile, None, fold)
        assert_counts_close(m, ref["mw"], R, T, 1e-10, f"{what}: m_step with multiplicities")
    if "em" in steps:
        got, info = d.em_run(None, N_ITER, 0.0, 50)
        launched("em_run", tile, None, fold)
        assert info.niter == N_ITER, (what, info)
        assert_counts_close(got, ref["em"], R, T, 1e-9, f"{what}: em_run")
        assert abs(got.sum() - R) < 1e-7 * R, (what, got.sum())
    for batched in (1, 0):
        if f"boot{batched}" not in steps:
            continue
        d.set_option(_lib.OEM_OPT_BATCH_BOOTSTRAP, batched)
        got, infos = d.bootstrap(N_REP, row_w_all=boot_w, max_iter=N_ITER, conv_thresh=0.0)
        if batched and batch is not None:
            launched("batched bootstrap", None, batch, False)      # (its fold, k_remote_fold_b, has one form)
        else:
            launched(f"bootstrap, batch option {batched}", tile, None, fold)
        for b in range(N_REP):
            assert infos[b].niter == N_ITER, (what, batched, b, infos[b])
            assert_counts_close(got[b], ref["boots"][b], R, T, 1e-9, f"{what}: batch option {batched}, replicate {b}")
            assert abs(got[b].sum() - R) < 1e-7 * R, (what, batched, b, got[b].sum())


# ---- the matrix ----------------------------------------------------------------------------------------------------------
CASES = list(itertools.product(STORES, VARIANTS, WINDOWS, (0, 1)))


@pytest.mark.parametrize("store,variant,window,nt", CASES, ids=["-".join(map(str, c[:3])) + f"-nt{c[3]}" for c in CASES])
def test_every_instantiation_matches_the_oracle(store, variant, window, nt, monkeypatch):
    _clear_knobs(monkeypatch)
    _set_nt(monkeypatch, nt)
    _one_chain(monkeypatch)
    _RAN.add((store, variant, window, nt))
    packed = 0 if store == "unpacked" else 1
    wide = 1 if window == "wide" else 0
    tile = (wide, *TILE[variant, window], packed, nt, 0)
    batch = None if wide else (*BATCH[variant], packed, nt)
    ref = _reference(store, variant)
    with _lib.testing(), _open(store, variant, window) as d:
        _run_case(d, ref, store, f"{store}/{variant}/{window}/nt={nt}", tile, batch, nt)


@pytest.mark.parametrize("store,variant,window", [c[:3] for c in CASES if c[3] == 0],
                         ids=["-".join(c[:3]) for c in CASES if c[3] == 0])
def test_cached_and_non_temporal_loads_give_the_same_pass(store, variant, window, monkeypatch):
    """The same store, the same pass: kNT changes how the streams are loaded and nothing of what is summed."""
    _clear_knobs(monkeypatch)
    row_ptr, _, _, T = _csr(store)
    theta, row_w, _ = _inputs(store)
    res = {}
    with _lib.testing(), _open(store, variant, window) as d:
        for nt in (0, 1):
            _set_nt(monkeypatch, nt)
            _last_launch(d)
            res[nt] = d.m_step(theta, row_w)
            tile, _, fold = _last_launch(d)
            assert tile is not None and tile[4] == nt and (fold is None or fold[0] == nt), (tile, fold)
    assert_counts_close(res[1], res[0], len(row_ptr) - 1, T, 1e-12, f"{store}/{variant}/{window}: nt against cached")


def test_without_knobs_a_small_store_takes_the_cached_streams_and_the_non_temporal_fold(monkeypatch):
    """The default dispatch is by size: below 96 MiB of streams kNT = false and kNTQ = true, in all three launchers."""
    _clear_knobs(monkeypatch)
    ref = _reference("remote", "fused")
    with _lib.testing(), _open("remote", "fused", "narrow") as d:
        tile, batch = (0, 0, FUSED, 1, 0, 0), (0, 1, 1, 0)
        _run_case(d, ref, "remote", "remote/fused, no knobs", tile, batch, 1, steps=("m", "boot1"))


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("knob,variant,tile_fc,batch_ff", [
    ("OEM_DICT_NO_FUSE", "fused", (0, BYTES), (0, 0)),   # <= 128 values, index bytes in a stream of their own
    ("OEM_NO_DICT", "bytes", (0, PLAIN), (0, 0)),        # a byte-coded store read through its f32 stream
    ("OEM_NO_DICT", "words", (0, PLAIN), (0, 0)),        # a word-coded store likewise
])
def test_coding_knobs_reach_the_byte_codes_and_the_f32_stream_of_a_coded_store(knob, variant, tile_fc, batch_ff, nt, monkeypatch):
    _clear_knobs(monkeypatch)
    _set_nt(monkeypatch, nt)
    monkeypatch.setenv(knob, "1")
    _one_chain(monkeypatch)
    ref = _reference("long", variant)
    with _lib.testing(), _open("long", variant, "narrow") as d:
        assert d.info(_lib.OEM_INFO_WEIGHT_DICT_ENTRIES) > 0          # coded all the same
        _run_case(d, ref, "long", f"long/{variant}/{knob}/nt={nt}", (0, *tile_fc, 1, nt, 0), (*batch_ff, 1, nt), nt,
                  steps=("m", "mw", "em", "boot1"))


# ---- the per-cell batch: problems != nullptr (tile index remap, live-tile list) ---------------------------------------
CELL_T = 3_000
CELL_READS = [2_000, 700, 1, 0, 1_500, 64, 65, 1_023, 1_025, 300, 2_500, 7]    # ragged; cell 3 is empty
CELL_ITER = 60     # with em::em's gate of 50 some cells converge and leave the live list, the others run into max_iter


@functools.lru_cache(maxsize=None)
def _cells():
    rps, tids, ps = [np.zeros(1, np.uint64)], [], []
    cell_off = np.zeros(len(CELL_READS) + 1, np.uint64)
    base = 0
    for c, n in enumerate(CELL_READS):
        cell_off[c + 1] = cell_off[c] + np.uint64(n)
        if n == 0:
            continue
        st = synth.make_store(n, CELL_T if c % 2 else CELL_T // 10, seed=500 + c, threads=1)
        rps.append(st.row_ptr[1:] + np.uint64(base))
        tids.append(st.tid)
        ps.append(st.as_prob)
        base += st.nnz
    return cell_off, np.concatenate(rps), np.concatenate(tids), np.concatenate(ps)


@functools.lru_cache(maxsize=None)
def _cell_weights(weights):
    _, _, tid, p = _cells()
    rng = np.random.default_rng(31)
    if weights == "coded":       # the generator's values: fused under the narrow cap, bytes under the wide one
        return p, None
    if weights == "plain":       # more than 1024 distinct values: the f32 stream
        return rng.uniform(1e-3, 1.0, size=len(tid)).astype(np.float32), None
    return p, rng.uniform(1e-3, 1.0, size=len(tid))


@functools.lru_cache(maxsize=None)
def _cell_reference(weights):
    cell_off, row_ptr, tid, _ = _cells()
    p, cov = _cell_weights(weights)
    out = []
    for c in range(len(CELL_READS)):
        r0, r1 = int(cell_off[c]), int(cell_off[c + 1])
        a0, a1 = int(row_ptr[r0]), int(row_ptr[r1])
        o = c_oracle.Store(row_ptr[r0:r1 + 1] - row_ptr[r0], tid[a0:a1], p[a0:a1], None if cov is None else cov[a0:a1], CELL_T)
        out.append(c_oracle.do_em(o, max_iter=CELL_ITER, conv_thresh=1e-3, min_iter_gate=50))
    return out


CELL_TILE = {("coded", "narrow"): (0, FUSED), ("coded", "wide"): (0, BYTES), ("plain", "narrow"): (0, PLAIN),
             ("plain", "wide"): (0, PLAIN), ("f64", "narrow"): (1, PLAIN), ("f64", "wide"): (1, PLAIN)}


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("weights", ["coded", "plain", "f64"])
def test_per_cell_batch_matches_the_per_cell_oracle_on_every_instantiation(weights, window, nt, monkeypatch):
    """12 ragged cells, one of them empty, as one batched store (oem_em_run_cells): every cell against em::em on its
    own store, as test_cells_match_per_cell_oracle.  A per-cell batch of this size takes the narrow cap by itself;
    OEM_WINDOW_CAP of the test-only library gives it the wide one that large batches run with."""
    _clear_knobs(monkeypatch)
    _set_nt(monkeypatch, nt)
    monkeypatch.setenv("OEM_WINDOW_CAP", "2048" if window == "wide" else "512")
    cell_off, row_ptr, tid, _ = _cells()
    p, cov = _cell_weights(weights)
    with _lib.testing():
        out, infos = oarfish_amd.em_cells(cell_off, row_ptr, tid, p, cov, CELL_T, max_iter=CELL_ITER, convergence_thresh=1e-3)
        tile, batch, fold = _last_launch()
    _RAN.add(("cells", weights, window, nt))
    want_tile = (1 if window == "wide" else 0, *CELL_TILE[weights, window], 1, nt, 1)
    # (no k_remote_fold: a per-cell batch folds its queue in the kernel that also takes its stopping decisions)
    assert (tile, batch, fold) == (want_tile, None, None), (tile, batch, fold)
    want = _cell_reference(weights)
    assert not out[3].any()
    for c, n in enumerate(CELL_READS):
        assert_cell_matches_oracle(infos[c], want[c], n, CELL_T, f"cells/{weights}/{window}/nt={nt}: cell {c}", dense=out[c])


# ---- completeness --------------------------------------------------------------------------------------------------------
def test_the_module_ran_every_reachable_instantiation():
    """Collected from the records of the tests above: the variants that ran are exactly the reachable ones.  It is a
    statement about the whole module, so it is made only when the whole matrix and every per-cell case ran in this
    process before it (not under -k, --lf or a split over workers: a partial set would read like a kernel gap)."""
    n_all = len(CASES) + 2 * len(CELL_TILE)
    if len(_RAN) != n_all:
        pytest.skip(f"{len(_RAN)} of the module's {n_all} matrix and per-cell cases ran in this process: run the whole module")
    assert _SEEN["tile"] == REACHABLE_TILE, (sorted(REACHABLE_TILE - _SEEN["tile"]), sorted(_SEEN["tile"] - REACHABLE_TILE))
    assert _SEEN["batch"] == REACHABLE_BATCH, (sorted(REACHABLE_BATCH - _SEEN["batch"]), sorted(_SEEN["batch"] - REACHABLE_BATCH))
    assert _SEEN["fold"] == REACHABLE_FOLD, _SEEN["fold"]
    want_cells = {(w, *CELL_TILE[k, win], 1, nt) for (k, win) in CELL_TILE for w in [1 if win == "wide" else 0] for nt in (0, 1)}
    assert _SEEN["cells"] == want_cells, (sorted(want_cells - _SEEN["cells"]), sorted(_SEEN["cells"] - want_cells))
