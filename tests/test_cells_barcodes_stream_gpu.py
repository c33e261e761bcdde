"""GPU tests of the barcoded cells session (oem_cells_stream_set_barcodes / _push_barcodes): however a barcode-collated
stream is cut into batches, finish gives what the one call over the cells (oem_em_run_cells_records_names_sparse) gives on
the surviving records with the cells the rule of oem_collate.h cuts -- cell_rec_off, order (as indices into the pushed
stream), group_off, cell_group_off, kept, the discard tables, the entries' offsets and columns and the labels exactly,
values and infos by the rule tests/test_collate_gpu.py holds a session to its one call with (_same_cells)."""
import ctypes as C
import itertools
import threading

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth, writers
from oarfish_amd.builder import ALN_RECORD
from oarfish_amd.single_cell import SingleCellArgs, quantify_single_cell_from_record_batches
from tests.test_cells_records_gpu import COVS
from tests.test_cells_records_names_gpu import _one_call, pack
from tests.test_collate_gpu import MAX_ITER, T, _same_cells

pytestmark = pytest.mark.gpu

U = _lib.REC_UNMAPPED
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 3001]
P9, Q9 = b"AAAAAAAAC", b"AAAAAAAAG"
GARBAGE = b"\x00\xff"


# ---- a stream: one entry per record --------------------------------------------------------------------------------------
def _stream(rec, bc, nm, sec):
    return dict(rec=np.ascontiguousarray(rec, dtype=ALN_RECORD), bc=list(bc), nm=list(nm), sec=np.asarray(sec, dtype=np.uint8))


def _unpack(pair):
    blob, off = pair
    raw, off = np.asarray(blob, dtype=np.uint8).tobytes(), np.asarray(off, dtype=np.int64)
    return [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def _lead(st, k):
    """k unmapped records in front, with bytes no survivor may carry"""
    head = np.zeros(k, dtype=ALN_RECORD)
    head["flags"] = U
    return _stream(np.concatenate([head, st["rec"]]), [GARBAGE] * k + st["bc"], [GARBAGE] * k + st["nm"],
                   np.concatenate([np.ones(k, dtype=np.uint8), st["sec"]]))


def _cut(st, edges):
    return [(st["rec"][a:b], st["bc"][a:b], st["nm"][a:b], st["sec"][a:b]) for a, b in zip(edges[:-1], edges[1:])]


def _cycled(n, sizes=SIZES):
    edges = [0]
    for s in itertools.cycle(sizes):
        if edges[-1] + s >= n:
            break
        edges.append(edges[-1] + s)
    return edges + [n]


def _walk(st):
    """the rule of oem_collate.h on the host: S, cell_rec_off among the survivors, the labels"""
    S = np.flatnonzero((st["rec"]["flags"] & U) == 0)
    cro, labels = [], []
    for k, i in enumerate(S):
        if not labels or st["bc"][i] != labels[-1]:
            cro.append(k)
            labels.append(st["bc"][i])
    return S, np.array(cro + [len(S)], dtype=np.uint64), labels


def _expected(st, filters, tl, model=-1, mode="sort", max_iter=MAX_ITER):
    """the one call on the survivors, and its order as indices into the stream"""
    S, cro, labels = _walk(st)
    want = _one_call(filters, tl, st["rec"][S], pack([st["nm"][i] for i in S]), st["sec"][S], cro, model=model, mode=mode,
                     max_iter=max_iter)
    want.update(order64=S.astype(np.uint64)[want["order"].astype(np.int64)], cell_rec_off=cro, barcodes=labels,
                n_unmapped=len(st["rec"]) - len(S), S=S)
    return want


def _session(batches, filters, tl, model=-1, mode="sort", max_iter=MAX_ITER, push=None, **opts):
    with oarfish_amd.CellsStream(len(tl), max_iter=max_iter, conv_thresh=1e-3, coverage=COVS[model],
                                 filters=filters, txp_len=tl, barcodes=True, mode=mode, **opts) as cs:
        if push is not None:
            push(cs)
        else:
            assert [cs.push_batch(*b) for b in batches] == list(range(len(batches)))
        cells = cs.finish()
        out = cs.cells()
        out.update(cells=cells, tables=cs.discard_tables(), info=cs.info())
    return out


def _same(got, want, label):
    assert got["barcodes"] == want["barcodes"], f"{label}: labels"
    assert got["n_unmapped"] == want["n_unmapped"], f"{label}: n_unmapped"
    for k, w in (("cell_rec_off", "cell_rec_off"), ("order", "order64"), ("group_off", "group_off"),
                 ("cell_group_off", "cell_group_off"), ("kept", "kept")):
        assert np.array_equal(got[k], want[w]), f"{label}: {k}"
    assert got["order"].dtype == np.uint64 and got["kept"].dtype == np.uint32
    assert got["tables"] == want["tables"], f"{label}: discard tables"
    _same_cells(got["cells"], want["cells"], label)       # indptr and columns exactly, values within 1 f32 ulp, the infos


# ---- 1. a hand-built input, every set of at most two cuts -----------------------------------------------------------------
EDGE_T = 40
EDGE_FILTERS = dict(five_prime_clip=2 ** 32 - 1, three_prime_clip=2 ** 62, score_threshold=0.95, min_aligned_fraction=0.5,
                    min_aligned_len=50, which_strand=0, score_prob_denom=5.0)
#            barcode    name     secondary  unmapped
INPUT16 = [(b"AAAA", b"r2", 0, 0), (b"AAAA", b"r1", 0, 0), (b"AAAA", b"r2", 1, 0), (b"", b"", 0, 1), (b"AAAA", b"r1", 1, 0),
           (b"CC", b"r1", 0, 0),                      # the same name next door: another cell, another read
           (GARBAGE, GARBAGE, 1, 1),                  # on a cell boundary
           (b"AAAA", b"solo", 0, 0),                  # the barcode comes back: a new cell, of one record
           (b"ACGT", b"x", 0, 0), (b"ACGT-1", b"x", 0, 0), (b"ACGT-1", b"y", 1, 0), (b"ACGT-1", b"y", 0, 0),
           (P9, b"a", 0, 0), (P9, b"b", 0, 0), (Q9, b"a", 0, 0), (b"", GARBAGE, 0, 1)]


def _stream16():
    rng = np.random.default_rng(16)
    rec = np.zeros(16, dtype=ALN_RECORD)
    for i, (_, _, _, un) in enumerate(INPUT16):
        rec[i] = (int(rng.integers(0, EDGE_T)), 10, 1500, 1400, 1000 - int(rng.integers(0, 30)), 1500, U if un else _lib.REC_HAS_SCORE, 0)
    return _stream(rec, [b for b, *_ in INPUT16], [n for _, n, *_ in INPUT16], [s for *_, s, _ in INPUT16])


def test_every_cutting_of_a_hand_built_input_at_up_to_two_positions():
    st, tl = _stream16(), np.full(EDGE_T, 2000, dtype=np.uint64)
    want = _expected(st, EDGE_FILTERS, tl, max_iter=20)
    assert want["barcodes"] == [b"AAAA", b"CC", b"AAAA", b"ACGT", b"ACGT-1", P9, Q9] and want["n_unmapped"] == 3
    assert list(want["cell_rec_off"]) == [0, 4, 5, 6, 7, 10, 12, 13]
    assert list(want["order64"][:4]) == [1, 4, 0, 2] and list(want["order64"][8:10]) == [11, 10]   # primary first
    cuttings = [c for k in (0, 1, 2) for c in itertools.combinations(range(1, 16), k)]
    assert len(cuttings) == 121
    for cuts in cuttings:
        got = _session(_cut(st, [0, *cuts, 16]), EDGE_FILTERS, tl, max_iter=20)
        _same(got, want, f"cuts {cuts}")


# ---- the fixture: about 40 cells, a few thousand records -----------------------------------------------------------------
READS = [30, 140, 9, 75, 51, 120, 1, 64, 33, 88, 17, 150, 42, 60, 5, 97, 28, 110, 70, 13, 56, 81, 24, 130, 47, 66, 3, 92, 38, 100,
         20, 58, 77, 11, 125, 45, 69, 26, 84, 35]
RECUR = (31, 12)      # cell 31 carries cell 12's label


@pytest.fixture(scope="module")
def base():
    stores = [synth.make_cells(1, r, T, kbar=4.0, seed=401 + k, expressed_frac=0.1 if k % 2 else None) for k, r in enumerate(READS)]
    co, rps, tids, ps, nnz = [0], [np.zeros(1, dtype=np.uint64)], [], [], 0
    for _, rp, tid, p in stores:
        rps.append(rp[1:] + np.uint64(nnz))
        tids.append(tid)
        ps.append(p)
        nnz += len(tid)
        co.append(co[-1] + len(rp) - 1)
    cr = synth.make_cell_records((np.array(co, dtype=np.uint64), np.concatenate(rps), np.concatenate(tids), np.concatenate(ps)),
                                 T, seed=11)
    bcs = synth.make_barcodes(len(READS))
    bcs[RECUR[0]] = bcs[RECUR[1]]
    return dict(cr=cr, filters=cr.filters, txp_len=cr.txp_len, bcs=bcs, streams={}, refs={})


def _sprinkled(rec, names, sec, cro, bcs, edges_of):
    """The input with an unmapped record in front of every seventh record, and as many more in front of everything as
    put one of the cycled cuts on a cell boundary."""
    (r, bc, nm, s), = synth.cut_cell_records(rec, names, sec, cro, bcs, (), unmapped_every=7)
    st = _stream(r, _unpack(bc), _unpack(nm), s)
    S, c, _ = _walk(st)
    firsts = S[c[1:-1].astype(np.int64)]            # the cells' first records, as stream positions
    lead = min((int(e - f) for e in edges_of(len(st["rec"]) + 64)[1:-1] for f in firsts if 0 <= e - f < 64), default=None)
    assert lead is not None
    return _lead(st, lead)


def _fixture_stream(base, style, mode):
    key = (style, mode)
    if key not in base["streams"]:
        rec, names, sec, cro = synth.shuffle_cell_records(base["cr"], seed=5, style=style)
        if mode == "adjacent":    # name-collated: every cell in the order the sort gives it
            nm = _unpack(names)
            order, _, _ = oarfish_amd.collate_names(names, cro, sec)
            order = order.astype(np.int64)
            rec, names, sec = rec[order], pack([nm[i] for i in order]), np.asarray(sec)[order]
        st = _sprinkled(rec, names, sec, cro, base["bcs"], _cycled)
        st["rec"].setflags(write=False)
        base["streams"][key] = st
    return base["streams"][key]


def _ref(base, style, model, mode):
    """The one call on the fixture's survivors, computed once and left alone; the conditions on the fixture."""
    key = (style, model, mode)
    if key not in base["refs"]:
        st = _fixture_stream(base, style, mode)
        ref = _expected(st, base["filters"], base["txp_len"], model, mode)
        n, S, cro = len(st["rec"]), ref["S"], ref["cell_rec_off"].astype(np.int64)
        assert len(cro) - 1 == len(READS) and 2000 < n < 20000 and ref["n_unmapped"] > n // 8
        assert ref["barcodes"][RECUR[0]] == ref["barcodes"][RECUR[1]]
        if mode == "sort":
            assert not np.array_equal(ref["order"], np.arange(len(S))), "the order is the identity: nothing is gathered"
        assert int((ref["kept"] > 0).sum()) > 0.9 * len(ref["kept"]), "the filter dropped the reads"
        # where the cycled cuts fall: by the survivors on either side of a cut
        cell_of = np.searchsorted(cro, np.arange(len(S)), side="right") - 1
        rank = np.searchsorted(S, np.arange(n + 1))           # survivors before a stream position
        un = (st["rec"]["flags"] & U) != 0
        inside_cell = on_boundary = inside_read = on_unmapped = 0
        for e in _cycled(n)[1:-1]:
            k = rank[e]
            if 0 < k < len(S):
                same = cell_of[k - 1] == cell_of[k]
                inside_cell += same
                on_boundary += (not same) and not un[e]        # the batch starts with the new cell's first record
                inside_read += same and st["nm"][S[k - 1]] == st["nm"][S[k]]
            on_unmapped += un[e]
        assert inside_cell and on_boundary and on_unmapped, (inside_cell, on_boundary, on_unmapped)
        if mode == "adjacent":
            assert inside_read, "no cut falls inside a read"
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        base["refs"][key] = ref
    return base["refs"][key]


# ---- 2. the fixture in cycled batch sizes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sort", "adjacent"])
@pytest.mark.parametrize("model", [-1, 1])
@pytest.mark.parametrize("style", ["uuid", "illumina"])
def test_cycled_batch_sizes_equal_the_one_call(base, style, model, mode):
    st = _fixture_stream(base, style, mode)
    want = _ref(base, style, model, mode)
    batches = _cut(st, _cycled(len(st["rec"])))
    assert {len(b[0]) for b in batches[:-1]} == set(SIZES)
    got = _session(batches, base["filters"], base["txp_len"], model, mode)
    _same(got, want, f"{style}, model {model}, {mode}")
    assert got["info"]["cells"] == len(batches) and got["info"]["alignments"] == len(st["rec"])


# ---- 3. one record per batch ----------------------------------------------------------------------------------------------
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
    _same(_session(_cut(st, list(range(301))), EDGE_FILTERS, tl, max_iter=20), want, "one record per batch")


# ---- 4. many groups under back-pressure -----------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [-1, 1])
def test_many_groups_under_back_pressure(base, model):
    st = _fixture_stream(base, "uuid", "sort")
    want = _ref(base, "uuid", model, "sort")
    batches = _cut(st, list(range(0, len(st["rec"]), 200)) + [len(st["rec"])])
    got = _session(batches, base["filters"], base["txp_len"], model, group_cells=2, max_staged_nnz=300)
    _same(got, want, f"group_cells = 2, model {model}")
    assert got["info"]["groups"] >= len(READS) // 2 and got["info"]["groups_before_finish"] > 0


# ---- 5. four pushing threads: the tickets give the order ------------------------------------------------------------------
def test_four_threads_push_and_the_tickets_give_the_order(base):
    st = _fixture_stream(base, "illumina", "sort")
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


# ---- 6. errors found on the device ----------------------------------------------------------------------------------------
def _fails(batches, at, code, words, filters=EDGE_FILTERS, n_txps=EDGE_T):
    """the error comes out of finish (or of a push behind the faulty batch), with these words, and sticks"""
    tl = np.full(n_txps, 2000, dtype=np.uint64)
    with oarfish_amd.CellsStream(n_txps, max_iter=20, filters=filters, txp_len=tl, barcodes=True) as cs:
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
    edges = [0, 5, 9, 13, 16]
    i = 10                                                  # in the third batch; record 3, 6 and 15 are unmapped and as bad
    st["bc" if what == "barcode" else "nm"][i] = bad
    words = [f"record {i} has an empty {what}"] if not bad else [f"the {what} of record {i} contains a 0 byte"]
    _fails(_cut(st, edges), 2, _lib.OEM_ERR_ARG, ["oem_cells_stream", "ticket 2"] + words)


@pytest.mark.parametrize("i, where", [(1, "a closed cell"), (14, "the carried cell")])
def test_a_bad_ref_id_names_ticket_and_session_index(i, where):
    st = _stream16()
    st["rec"]["ref_id"][i] = EDGE_T
    ticket = 0 if i < 5 else 3
    _fails(_cut(st, [0, 5, 9, 13, 16]), 3, _lib.OEM_ERR_ARG,
           ["oem_cells_stream", f"ticket {ticket}", f"record {i}:", f"ref_id {EDGE_T} is not below n_txps"])


# ---- 7. the host loop -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["big_score", "zero_denom"])
def test_host_loop_fallbacks(base, case):
    full = _fixture_stream(base, "uuid", "sort")
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
    _same(_session(_cut(st, _cycled(n, [1, 64, 257, 100])), filters, base["txp_len"], group_cells=3), want, case)


# ---- 8. session behaviour -------------------------------------------------------------------------------------------------
def test_empty_and_unmapped_only_sessions():
    tl = np.full(EDGE_T, 2000, dtype=np.uint64)
    got = _session([], EDGE_FILTERS, tl)
    assert got["barcodes"] == [] and list(got["cell_rec_off"]) == [0] and list(got["group_off"]) == [0] and got["n_unmapped"] == 0
    assert len(got["order"]) == 0 and len(got["kept"]) == 0 and list(got["cells"][0]) == [0] and got["tables"] == []
    st = _lead(_stream(np.zeros(0, dtype=ALN_RECORD), [], [], []), 5)
    got = _session(_cut(st, [0, 0, 2, 5]), EDGE_FILTERS, tl)
    assert got["barcodes"] == [] and got["n_unmapped"] == 5 and list(got["cells"][0]) == [0] and got["info"]["cells"] == 3


def test_call_order_errors_and_destroy_with_staged_batches():
    L = _lib.lib()
    tl = np.full(EDGE_T, 2000, dtype=np.uint64)
    st = _stream16()
    goff = np.array([0, 16], dtype=np.uint64)
    t = C.c_uint64(0)
    with oarfish_amd.CellsStream(EDGE_T, filters=EDGE_FILTERS, txp_len=tl, barcodes=True) as cs:   # wrong-kind pushes
        with pytest.raises(oarfish_amd.OemError) as ei:
            cs.push_records(st["rec"], goff)
        assert ei.value.code == _lib.OEM_ERR_STATE and "barcoded session" in str(ei.value)
        rp = np.zeros(1, dtype=np.uint64)
        assert L.oem_cells_stream_push(cs._h, rp.ctypes.data, None, None, None, None, 0, 0, C.byref(t)) == _lib.OEM_ERR_STATE
        assert L.oem_cells_stream_set_barcodes(cs._h, 0) == _lib.OEM_ERR_STATE and b"already" in L.oem_last_error()
        assert L.oem_cells_stream_barcodes_dims(cs._h, None, None, None, None, None) == _lib.OEM_ERR_STATE     # not finished
        cs.push_batch(*_cut(st, [0, 16])[0])
        cs.finish()
        with pytest.raises(oarfish_amd.OemError) as ei:          # finish twice
            cs.finish()
        assert ei.value.code == _lib.OEM_ERR_STATE
        with pytest.raises(oarfish_amd.OemError) as ei:
            cs.push_batch(*_cut(st, [0, 16])[0])
        assert ei.value.code == _lib.OEM_ERR_STATE
        blob = np.zeros(64, dtype=np.uint8)
        assert L.oem_cells_stream_barcodes_copy(cs._h, blob.ctypes.data, None, None, None, None, None, None) == _lib.OEM_ERR_ARG
    with oarfish_amd.CellsStream(EDGE_T, filters=EDGE_FILTERS, txp_len=tl) as cs:                  # a records session
        with pytest.raises(oarfish_amd.OemError) as ei:
            cs.push_batch(*_cut(st, [0, 16])[0])
        assert ei.value.code == _lib.OEM_ERR_STATE and "not a barcoded session" in str(ei.value)
        assert L.oem_cells_stream_barcodes_dims(cs._h, None, None, None, None, None) == _lib.OEM_ERR_STATE
        assert L.oem_cells_stream_barcodes_copy(cs._h, None, None, None, None, None, None, None) == _lib.OEM_ERR_STATE
        assert L.oem_cells_stream_set_barcodes(cs._h, 2) == _lib.OEM_ERR_ARG
        cs.push_records(st["rec"], goff)
        assert L.oem_cells_stream_set_barcodes(cs._h, 0) == _lib.OEM_ERR_STATE                     # after a push
    with oarfish_amd.CellsStream(EDGE_T) as cs:                                                    # a plain session
        assert L.oem_cells_stream_set_barcodes(cs._h, 0) == _lib.OEM_ERR_STATE
    cs = oarfish_amd.CellsStream(EDGE_T, filters=EDGE_FILTERS, txp_len=tl, barcodes=True)          # destroy with staged batches
    for b in _cut(st, [0, 3, 8, 16]) * 20:
        cs.push_batch(*b)
    cs.close()


# ---- 9. the driver --------------------------------------------------------------------------------------------------------
def test_the_driver_writes_the_files_of_the_one_call(base, tmp_path):
    st = _fixture_stream(base, "illumina", "sort")
    want = _ref(base, "illumina", 1, "sort")
    names = [f"t{i}" for i in range(T)]
    args = SingleCellArgs(output=str(tmp_path / "stream" / "out"), max_em_iter=MAX_ITER, model_coverage="binomial")
    got = quantify_single_cell_from_record_batches(base["filters"], names, base["txp_len"], _cut(st, _cycled(len(st["rec"]))), args)
    assert got[4]["barcodes"] == want["barcodes"]
    ref_out = str(tmp_path / "onecall" / "out")
    info = {"output": args.output, "single_cell": True, "em_max_iter": MAX_ITER, "em_convergence_thresh": 1e-3, "threads": 3,
            "filter_options": {"model_coverage": True}}
    indptr, cols, vals, _ = want["cells"]
    # (with the session's default budgets the fixture's cells are one group, as in the one call: the same tiles, the same bits)
    writers.write_single_cell_output_device(ref_out, info, names, [b.decode("latin-1") for b in want["barcodes"]], len(READS), indptr,
                                            cols, vals)
    for ext in (".count.mtx", ".features.txt", ".barcodes.txt", ".meta_info.json"):
        a, b = open(args.output + ext, "rb").read(), open(ref_out + ext, "rb").read()
        assert a == b and len(a) > 0, ext
    assert open(args.output + ".barcodes.txt").read().split() == [b.decode() for b in want["barcodes"]]
