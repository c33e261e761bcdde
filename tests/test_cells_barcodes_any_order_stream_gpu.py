"""GPU tests of the any-order barcoded cells session (oem_cells_stream_set_barcodes_any_order): however a stream of records
in any order is cut into batches, finish gives what the one call (oem_em_run_cells_records_barcodes_sparse, what
em_cells_records_sparse(..., names=, secondary=, barcodes=, collate="device") calls) gives on the surviving records --
cell_rec_off, order (as indices into the pushed stream), group_off, cell_group_off, kept, the discard tables, the entries'
offsets and columns and the labels exactly, values and infos by the rule tests/test_collate_gpu.py holds a session to its
one call with (_same_cells).  The expected side never comes from the session."""
import ctypes as C
import itertools
import threading

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth, writers
from oarfish_amd.builder import ALN_RECORD
from oarfish_amd.single_cell import SingleCellArgs, quantify_single_cell_from_record_batches
from tests.test_cells_barcodes_stream_gpu import (EDGE_FILTERS, EDGE_T, GARBAGE, P9, Q9, READS, SIZES, U, _cut, _cycled, _lead, _same,
                                                  _stream, _unpack, base)   # noqa: F401  (base: the module's fixture)
from tests.test_cells_records_gpu import COVS
from tests.test_cells_records_names_gpu import pack
from tests.test_collate_barcodes_gpu import _one_call as _barcodes_call
from tests.test_collate_gpu import MAX_ITER, T

pytestmark = pytest.mark.gpu

C8 = b"CCCCCCCC"


# ---- the two sides ---------------------------------------------------------------------------------------------------------
def _expected(st, filters, tl, model=-1, mode="sort", max_iter=MAX_ITER):
    """the one call on the survivors, its order as indices into the stream, the labels from the cells' first records"""
    S = np.flatnonzero((st["rec"]["flags"] & U) == 0)
    want = _barcodes_call(filters, tl, st["rec"][S], pack([st["nm"][i] for i in S]), st["sec"][S], pack([st["bc"][i] for i in S]),
                          model=model, mode=mode, max_iter=max_iter)
    order64 = S.astype(np.uint64)[want["order"].astype(np.int64)]
    cro = want["cell_rec_off"].astype(np.int64)
    want.update(order64=order64, barcodes=[st["bc"][int(order64[c])] for c in cro[:-1]], n_unmapped=len(st["rec"]) - len(S), S=S)
    seen = list(dict.fromkeys(st["bc"][i] for i in S))
    assert want["barcodes"] == seen                         # cells are numbered by their first survivor
    return want


def _session(batches, filters, tl, model=-1, mode="sort", max_iter=MAX_ITER, push=None, **opts):
    with oarfish_amd.CellsStream(len(tl), max_iter=max_iter, conv_thresh=1e-3, coverage=COVS[model],
                                 filters=filters, txp_len=tl, barcodes=True, collated=False, mode=mode, **opts) as cs:
        if push is not None:
            push(cs)
        else:
            assert [cs.push_batch(*b) for b in batches] == list(range(len(batches)))
        before = cs.info()
        cells = cs.finish()
        out = cs.cells()
        out.update(cells=cells, tables=cs.discard_tables(), info=cs.info(), before=before)
    assert out["info"]["groups_before_finish"] == 0         # nothing runs before finish: any barcode may return
    return out


def _misses(batches):
    """per batch, from the input alone: (survivors, survivors whose barcode no earlier batch has, a new label's first
    survivor comes after an old label's survivor)"""
    seen, out = set(), []
    for rec, bc, _, _ in batches:
        surv = [bc[i] for i in np.flatnonzero((rec["flags"] & U) == 0)]
        miss = [b not in seen for b in surv]
        late = any(m and not all(miss[:k]) and b not in surv[:k] for k, (b, m) in enumerate(zip(surv, miss)))
        out.append((len(surv), sum(miss), late))
        seen.update(surv)
    return out


def _table_growth(batches, slots0):
    """from the input alone: (final capacity, batches that rebuilt the table, the most doublings in one of them)"""
    seen, cap, rebuilds, most = set(), slots0, 0, 0
    for rec, bc, _, _ in batches:
        seen.update(bc[i] for i in np.flatnonzero((rec["flags"] & U) == 0))
        d = 0
        while 2 * len(seen) > cap:
            cap, d = 2 * cap, d + 1
        rebuilds, most = rebuilds + (d > 0), max(most, d)
    return cap, rebuilds, most


def _check_info(got, batches, n_labels):
    per = _misses(batches)
    info = got["info"]
    assert info["barcode_misses"] == sum(m for _, m, _ in per)
    slots = info["barcode_table_slots"]
    assert slots >= 2 * n_labels and slots & (slots - 1) == 0
    n_surv = sum(s for s, _, _ in per)
    assert info["arena_bytes"] >= n_surv * (40 + 8 + 8 + 1 + 4) and got["before"]["arena_bytes"] <= info["arena_bytes"]
    assert info["cells"] == len(batches)
    return per


# ---- 1. a hand-built input, every set of at most two cuts -----------------------------------------------------------------
#            barcode    name     secondary  unmapped
INPUT16 = [(GARBAGE, GARBAGE, 1, 1), (b"T", b"r2", 0, 0), (C8, b"r1", 0, 0), (b"ACGT-1", b"x", 0, 0), (b"T", b"r1", 0, 0),
           (b"ACGT", b"x", 0, 0), (b"T", b"r2", 1, 0), (Q9, b"a", 0, 0), (b"", b"", 0, 1), (P9, b"a", 0, 0), (b"ACGT-1", b"y", 1, 0),
           (b"T", b"r1", 1, 0), (Q9, b"b", 0, 0), (b"ACGT-1", b"y", 0, 0), (C8, b"r1", 1, 0), (b"", GARBAGE, 0, 1)]
LABELS16 = [b"T", C8, b"ACGT-1", b"ACGT", Q9, P9]


def _stream16():
    rng = np.random.default_rng(16)
    rec = np.zeros(16, dtype=ALN_RECORD)
    for i, (_, _, _, un) in enumerate(INPUT16):
        rec[i] = (int(rng.integers(0, EDGE_T)), 10, 1500, 1400, 1000 - int(rng.integers(0, 30)), 1500, U if un else _lib.REC_HAS_SCORE, 0)
    return _stream(rec, [b for b, *_ in INPUT16], [n for _, n, *_ in INPUT16], [s for *_, s, _ in INPUT16])


def test_every_cutting_of_a_hand_built_input_at_up_to_two_positions():
    st, tl = _stream16(), np.full(EDGE_T, 2000, dtype=np.uint64)
    want = _expected(st, EDGE_FILTERS, tl, max_iter=20)
    assert want["barcodes"] == LABELS16 == sorted(LABELS16, reverse=True) and want["n_unmapped"] == 3
    assert list(want["cell_rec_off"]) == [0, 4, 6, 9, 10, 12, 13]
    assert list(want["order64"][:4]) == [4, 11, 1, 6] and list(want["order64"][6:9]) == [3, 13, 10]   # by name, primary first
    cuttings = [c for k in (0, 1, 2) for c in itertools.combinations(range(1, 16), k)]
    assert len(cuttings) == 121
    for cuts in cuttings:
        batches = _cut(st, [0, *cuts, 16])
        got = _session(batches, EDGE_FILTERS, tl, max_iter=20)
        _same(got, want, f"cuts {cuts}")
        _check_info(got, batches, len(LABELS16))


# ---- 2. the fixture, interleaved, in cycled batch sizes --------------------------------------------------------------------
def _interleaved(base, style, how):
    key = ("any", style, how)
    if key not in base["streams"]:
        rec, names, sec, cro = synth.shuffle_cell_records(base["cr"], seed=5, style=style)
        irec, inames, isec, ibc, _ = synth.interleave_cells(rec, names, sec, cro, base["bcs"], seed=9, how=how)
        (r, bc, nm, s), = synth.cut_interleaved_records(irec, inames, isec, ibc, (), unmapped_every=7)
        bc, nm = _unpack(bc), _unpack(nm)
        for i in np.flatnonzero((r["flags"] & U) != 0):     # bytes no survivor may carry
            bc[i], nm[i] = GARBAGE, GARBAGE
        st = _stream(r, bc, nm, s)
        st["rec"].setflags(write=False)
        base["streams"][key] = st
    return base["streams"][key]


def _ref(base, style, how, model, mode):
    key = ("any", style, how, model, mode)
    if key not in base["refs"]:
        st = _interleaved(base, style, how)
        ref = _expected(st, base["filters"], base["txp_len"], model, mode)
        n = len(st["rec"])
        assert len(ref["barcodes"]) == len(set(base["bcs"])) == len(READS) - 1 and 2000 < n < 20000 and ref["n_unmapped"] > n // 8
        assert int((ref["kept"] > 0).sum()) > 0.5 * len(ref["kept"]), "the filter dropped the reads"
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        base["refs"][key] = ref
    return base["refs"][key]


@pytest.mark.parametrize("mode", ["sort", "adjacent"])
@pytest.mark.parametrize("model", [-1, 1])
@pytest.mark.parametrize("style", ["uuid", "illumina"])
@pytest.mark.parametrize("how", ["uniform", "blocks"])
def test_interleaved_fixture_in_cycled_batch_sizes_equals_the_one_call(base, how, style, model, mode):
    st = _interleaved(base, style, how)
    want = _ref(base, style, how, model, mode)
    batches = _cut(st, _cycled(len(st["rec"])))
    assert {len(b[0]) for b in batches[:-1]} == set(SIZES)
    got = _session(batches, base["filters"], base["txp_len"], model, mode)
    _same(got, want, f"{how}, {style}, model {model}, {mode}")
    per = _check_info(got, batches, len(want["barcodes"]))
    first = next(k for k, (s, _, _) in enumerate(per) if s)
    assert per[first][1] > 0 and any(s and not m for s, m, _ in per[first + 1:])   # misses first, later a batch without any
    assert any(late for _, _, late in per), "no batch has a new label behind an old one"
    assert got["info"]["barcode_misses"] < len(want["S"]) and got["info"]["alignments"] == len(st["rec"])


# ---- 3. 300 cells: the cell id needs a second radix digit -------------------------------------------------------------------
def _small_cells(n_cells, seed):
    rng = np.random.default_rng(seed)
    bcs = synth.make_barcodes(n_cells)
    bcs = [b.encode() if isinstance(b, str) else b for b in bcs]
    cell = np.repeat(np.arange(n_cells - 1), rng.integers(1, 4, size=n_cells - 1))
    cell = np.concatenate([rng.permutation(cell), [n_cells - 1]])           # one single-record cell last
    n = len(cell)
    rec = np.zeros(n, dtype=ALN_RECORD)
    for i in range(n):
        rec[i] = (int(rng.integers(0, EDGE_T)), 10, 1500, 1400, 1000 - int(rng.integers(0, 30)), 1500, _lib.REC_HAS_SCORE, 0)
    return _stream(rec, [bcs[c] for c in cell], [b"q%d" % v for v in rng.integers(0, 40, size=n)], rng.integers(0, 2, size=n))


def test_300_cells_of_one_to_three_records_with_a_single_record_cell_last():
    st, tl = _small_cells(300, 33), np.full(EDGE_T, 2000, dtype=np.uint64)
    want = _expected(st, EDGE_FILTERS, tl, max_iter=20)
    cro = want["cell_rec_off"].astype(np.int64)
    assert len(cro) == 301 and set(np.diff(cro)) == {1, 2, 3} and cro[-1] - cro[-2] == 1 and want["order64"][-1] == len(st["rec"]) - 1
    batches = _cut(st, _cycled(len(st["rec"]), [1, 7, 64, 100]))
    got = _session(batches, EDGE_FILTERS, tl, max_iter=20)
    _same(got, want, "300 cells")
    _check_info(got, batches, 300)


# ---- 4. one record per batch ------------------------------------------------------------------------------------------------
def test_one_cell_of_300_records_one_record_per_batch():
    rng = np.random.default_rng(300)
    rec = np.zeros(300, dtype=ALN_RECORD)
    for i in range(300):
        rec[i] = (int(rng.integers(0, EDGE_T)), 10, 1500, 1400, 1000 - int(rng.integers(0, 30)), 1500, _lib.REC_HAS_SCORE, 0)
    nm = [b"read/%d" % v for v in rng.integers(0, 100, size=300)]
    st = _stream(rec, [b"ACGTACGTACGTACGT-1"] * 300, nm, rng.integers(0, 2, size=300))
    tl = np.full(EDGE_T, 2000, dtype=np.uint64)
    want = _expected(st, EDGE_FILTERS, tl, max_iter=20)
    assert list(want["cell_rec_off"]) == [0, 300] and not np.array_equal(want["order"], np.arange(300))
    batches = _cut(st, list(range(301)))
    got = _session(batches, EDGE_FILTERS, tl, max_iter=20)
    _same(got, want, "one record per batch")
    assert got["info"]["barcode_misses"] == 1


# ---- 5. the table under the testing library's knobs ------------------------------------------------------------------------
@pytest.mark.parametrize("knob, value", [("OEM_BARCODE_HASH_BITS", "0"), ("OEM_BARCODE_TABLE_SLOTS0", "2")])
def test_a_masked_hash_and_a_first_capacity_of_two_give_the_same_result(base, monkeypatch, knob, value):
    st = _interleaved(base, "uuid", "uniform")
    want = _ref(base, "uuid", "uniform", -1, "sort")
    batches = _cut(st, _cycled(len(st["rec"])))
    monkeypatch.setenv(knob, value)
    with _lib.testing() as L:
        got = _session(batches, base["filters"], base["txp_len"])
        last = (C.c_uint64 * 8)()
        assert L.oem_debug_barcode_table_last(last) == _lib.OEM_OK
    _same(got, want, f"{knob} = {value}")
    n_labels = len(want["barcodes"])
    rebuilds, longest, wrapped, doublings, slots, labels, misses = list(last)[:7]
    assert labels == n_labels and misses == got["info"]["barcode_misses"] and slots == got["info"]["barcode_table_slots"]
    if knob == "OEM_BARCODE_HASH_BITS":      # every label's home is the last slot: every probe but one wraps, the longest sees all
        assert wrapped == 1 and longest >= n_labels and rebuilds == 0
    else:                                    # 2 slots to 128: across batches, and several doublings inside the batch of 63
        assert (slots, rebuilds, doublings) == _table_growth(batches, 2)
        assert slots == 128 and rebuilds >= 2 and doublings >= 2 and longest >= 1


# ---- 6. four pushing threads: the tickets give the order ------------------------------------------------------------------
def test_four_threads_push_and_the_tickets_give_the_order(base):
    st = _interleaved(base, "illumina", "blocks")
    batches = _cut(st, list(range(0, len(st["rec"]), 150)) + [len(st["rec"])])
    tickets = [None] * len(batches)

    def push(cs):
        def one(t):
            for k in range(t, len(batches), 4):
                tickets[k] = cs.push_batch(*batches[k])
        threads = [threading.Thread(target=one, args=(t,)) for t in range(4)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()

    got = _session(None, base["filters"], base["txp_len"], push=push)
    assert sorted(tickets) == list(range(len(batches)))
    by_ticket = [batches[k] for k in np.argsort(tickets)]
    pushed = _stream(np.concatenate([b[0] for b in by_ticket]), sum((b[1] for b in by_ticket), []), sum((b[2] for b in by_ticket), []),
                     np.concatenate([b[3] for b in by_ticket]))
    _same(got, _expected(pushed, base["filters"], base["txp_len"]), "four threads")


# ---- 7. errors found on the device ----------------------------------------------------------------------------------------
def _fails(batches, at, code, words):
    """the error comes out of finish (or of a push behind the faulty batch), with these words, and sticks"""
    tl = np.full(EDGE_T, 2000, dtype=np.uint64)
    with oarfish_amd.CellsStream(EDGE_T, max_iter=20, filters=EDGE_FILTERS, txp_len=tl, barcodes=True, collated=False) as cs:
        for b in batches[:at + 1]:
            cs.push_batch(*b)
        errors = []
        for b in batches[at + 1:]:
            try:
                cs.push_batch(*b)
            except oarfish_amd.OemError as e:
                errors.append(e)
        with pytest.raises(oarfish_amd.OemError) as ei:
            cs.finish()
        errors.append(ei.value)
        with pytest.raises(oarfish_amd.OemError) as again:      # sticky: a later push says the same
            cs.push_batch(*batches[0])
        errors.append(again.value)
        for e in errors:
            assert e.code == code and all(w in str(e) for w in words), str(e)
        assert str(errors[0]) == str(errors[-1])
        with pytest.raises(oarfish_amd.OemError):
            cs.cells()


@pytest.mark.parametrize("what, bad", [("barcode", b""), ("barcode", b"AC\x00T"), ("name", b""), ("name", b"r\x00")])
def test_a_bad_barcode_or_name_in_the_third_batch(what, bad):
    st = _stream16()
    i = 10                                                  # in the third batch; records 0, 8 and 15 are unmapped and as bad
    st["bc" if what == "barcode" else "nm"][i] = bad
    words = [f"record {i} has an empty {what}"] if not bad else [f"the {what} of record {i} contains a 0 byte"]
    _fails(_cut(st, [0, 5, 9, 13, 16]), 2, _lib.OEM_ERR_ARG, ["oem_cells_stream", "ticket 2"] + words)


def test_a_bad_ref_id_in_the_first_batch_and_another_in_the_last():
    st = _stream16()
    st["rec"]["ref_id"][2] = EDGE_T
    st["rec"]["ref_id"][14] = EDGE_T + 1
    # (the faulty batch is the first: every push behind it may meet the sticky error already)
    _fails(_cut(st, [0, 5, 9, 13, 16]), 0, _lib.OEM_ERR_ARG,
           ["oem_cells_stream", "ticket 0", "record 2:", f"ref_id {EDGE_T} is not below n_txps"])
    st = _stream16()
    st["rec"]["ref_id"][14] = EDGE_T + 1                    # the last batch alone: its own ticket, the session-global index
    _fails(_cut(st, [0, 5, 9, 13, 16]), 3, _lib.OEM_ERR_ARG,
           ["oem_cells_stream", "ticket 3", "record 14:", f"ref_id {EDGE_T + 1} is not below n_txps"])


# ---- 8. the host loop -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["big_score", "zero_denom"])
def test_host_loop_fallbacks(base, case):
    full = _interleaved(base, "uuid", "uniform")
    n = 3000
    st = _stream(full["rec"][:n].copy(), full["bc"][:n], full["nm"][:n], full["sec"][:n])
    filters = dict(base["filters"])
    if case == "big_score":
        i = int(np.flatnonzero((st["rec"]["flags"] & U) == 0)[1400])
        st["rec"]["score"][i] = 2 ** 24 + 1
        st["rec"]["flags"][i] |= _lib.REC_HAS_SCORE
    else:
        filters["score_prob_denom"] = 0.0
    want = _expected(st, filters, base["txp_len"])
    assert len(want["barcodes"]) > 5
    got = _session(_cut(st, _cycled(n, [1, 64, 257, 100])), filters, base["txp_len"], group_cells=3)
    _same(got, want, case)
    assert got["info"]["groups"] >= len(want["barcodes"]) // 3


# ---- 9. session behaviour -------------------------------------------------------------------------------------------------
def test_empty_and_unmapped_only_sessions():
    tl = np.full(EDGE_T, 2000, dtype=np.uint64)
    got = _session([], EDGE_FILTERS, tl)
    assert got["barcodes"] == [] and list(got["cell_rec_off"]) == [0] and list(got["group_off"]) == [0] and got["n_unmapped"] == 0
    assert len(got["order"]) == 0 and len(got["kept"]) == 0 and list(got["cells"][0]) == [0] and got["tables"] == []
    assert got["info"]["barcode_misses"] == 0 and got["info"]["arena_bytes"] == 0
    st = _lead(_stream(np.zeros(0, dtype=ALN_RECORD), [], [], []), 5)
    got = _session(_cut(st, [0, 0, 2, 5]), EDGE_FILTERS, tl)
    assert got["barcodes"] == [] and got["n_unmapped"] == 5 and list(got["cells"][0]) == [0] and got["info"]["cells"] == 3


def test_call_order_errors_and_close_with_staged_batches():
    L = _lib.lib()
    tl = np.full(EDGE_T, 2000, dtype=np.uint64)
    st = _stream16()
    goff = np.array([0, 16], dtype=np.uint64)
    with oarfish_amd.CellsStream(EDGE_T, filters=EDGE_FILTERS, txp_len=tl, barcodes=True, collated=False) as cs:
        assert L.oem_cells_stream_set_barcodes(cs._h, 0) == _lib.OEM_ERR_STATE and b"already" in L.oem_last_error()
        assert L.oem_cells_stream_set_barcodes_any_order(cs._h, 0) == _lib.OEM_ERR_STATE and b"already" in L.oem_last_error()
        with pytest.raises(oarfish_amd.OemError) as ei:
            cs.push_records(st["rec"], goff)
        assert ei.value.code == _lib.OEM_ERR_STATE and "barcoded session" in str(ei.value)
        assert L.oem_cells_stream_barcodes_dims(cs._h, None, None, None, None, None) == _lib.OEM_ERR_STATE     # not finished
        cs.push_batch(*_cut(st, [0, 16])[0])
        cs.finish()
        assert L.oem_cells_stream_set_barcodes_any_order(cs._h, 0) == _lib.OEM_ERR_STATE                       # after finish
        with pytest.raises(oarfish_amd.OemError) as ei:
            cs.push_batch(*_cut(st, [0, 16])[0])
        assert ei.value.code == _lib.OEM_ERR_STATE
    with oarfish_amd.CellsStream(EDGE_T, filters=EDGE_FILTERS, txp_len=tl, barcodes=True) as cs:   # the other direction
        assert L.oem_cells_stream_set_barcodes_any_order(cs._h, 0) == _lib.OEM_ERR_STATE and b"already" in L.oem_last_error()
        assert cs.info()["arena_bytes"] == 0 and cs.info()["barcode_table_slots"] == 0
    with oarfish_amd.CellsStream(EDGE_T, filters=EDGE_FILTERS, txp_len=tl) as cs:                  # a records session
        assert L.oem_cells_stream_set_barcodes_any_order(cs._h, 2) == _lib.OEM_ERR_ARG
        cs.push_records(st["rec"], goff)
        assert L.oem_cells_stream_set_barcodes_any_order(cs._h, 0) == _lib.OEM_ERR_STATE           # after a push
    with oarfish_amd.CellsStream(EDGE_T) as cs:                                                    # a plain session
        assert L.oem_cells_stream_set_barcodes_any_order(cs._h, 0) == _lib.OEM_ERR_STATE
    cs = oarfish_amd.CellsStream(EDGE_T, filters=EDGE_FILTERS, txp_len=tl, barcodes=True, collated=False)
    for b in _cut(st, [0, 3, 8, 16]) * 20:                                                         # close with staged batches
        cs.push_batch(*b)
    cs.close()


# ---- 11. the driver -------------------------------------------------------------------------------------------------------
def test_the_driver_writes_the_files_of_the_one_call(base, tmp_path):
    st = _interleaved(base, "illumina", "uniform")
    want = _ref(base, "illumina", "uniform", 1, "sort")
    names = [f"t{i}" for i in range(T)]
    args = SingleCellArgs(output=str(tmp_path / "stream" / "out"), max_em_iter=MAX_ITER, model_coverage="binomial", collated=False)
    got = quantify_single_cell_from_record_batches(base["filters"], names, base["txp_len"], _cut(st, _cycled(len(st["rec"]))), args)
    assert got[4]["barcodes"] == want["barcodes"]
    ref_out = str(tmp_path / "onecall" / "out")
    info = {"output": args.output, "single_cell": True, "em_max_iter": MAX_ITER, "em_convergence_thresh": 1e-3, "threads": 3,
            "filter_options": {"model_coverage": True}}
    indptr, cols, vals, _ = want["cells"]
    # (with the session's default budgets the fixture's cells are one group, as in the one call: the same tiles, the same bits)
    writers.write_single_cell_output_device(ref_out, info, names, [b.decode("latin-1") for b in want["barcodes"]], len(want["barcodes"]),
                                            indptr, cols, vals)
    for ext in (".count.mtx", ".features.txt", ".barcodes.txt", ".meta_info.json"):
        a, b = open(args.output + ext, "rb").read(), open(ref_out + ext, "rb").read()
        assert a == b and len(a) > 0, ext
