"""GPU tests of the UMI sessions (oem_cells_stream_set_umis / _push_barcodes_umis / _umis_copy): the two barcoded cells
sessions with one UMI per record, deduplicated on the device behind every group's name collation.

The any-order form is held to the UMIs one call (oem_em_run_cells_records_umis_sparse) on the surviving records; the
collated form, where a barcode that comes back is a new cell, to the join of oem_collate.h's "UMIs in the sessions":
oem_collate_names with the streamed cells, oem_dedup_umis, the duplicates dropped, oem_em_run_cells_records_sparse.  Every
index array and count, kept, the discard tables, cell_dups, the labels and the columns are compared exactly, values and
infos by the rule tests/test_collate_gpu.py holds a session to its one call with.  The expected side never comes from a
session."""
import itertools
import threading

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth, writers
from oarfish_amd.builder import ALN_RECORD
from oarfish_amd.em import gather_names
from oarfish_amd.single_cell import SingleCellArgs, quantify_single_cell_from_record_batches
from tests.test_cells_barcodes_stream_gpu import (EDGE_FILTERS, EDGE_T, GARBAGE, P9, Q9, SIZES, U, _cycled, _same, _stream, _unpack,
                                                  _walk)
from tests.test_cells_records_gpu import COVS
from tests.test_cells_records_names_gpu import pack
from tests.test_collate_gpu import MAX_ITER, T
from tests.test_dedup_umis_gpu import _one_call as _umis_call, aug, base, inter   # noqa: F401  (aug, base, inter: fixtures)

pytestmark = pytest.mark.gpu

FORMS = [True, False]    # collated


# ---- a stream with UMIs, its cuttings, the two expected sides and the session ---------------------------------------------
def _ustream(rec, bc, nm, sec, um):
    st = _stream(rec, bc, nm, sec)
    st["um"] = list(um)
    return st


def _cut(st, edges):
    return [(st["rec"][a:b], st["bc"][a:b], st["nm"][a:b], st["sec"][a:b], st["um"][a:b]) for a, b in zip(edges[:-1], edges[1:])]


def _finish_want(st, S, want, order):
    order64 = S.astype(np.uint64)[np.asarray(order).astype(np.int64)]
    cro = np.asarray(want["cell_rec_off"]).astype(np.int64)
    want.update(order64=order64, barcodes=[st["bc"][int(order64[c])] for c in cro[:-1]], n_unmapped=len(st["rec"]) - len(S), S=S,
                dup_records=len(S) - len(order64), cell_dups=np.asarray(want["cell_dups"], dtype=np.uint64))
    return want


def _expected_any_order(st, filters, tl, model=-1, mode="sort", max_iter=MAX_ITER):
    """the UMIs one call on the survivors"""
    S = np.flatnonzero((st["rec"]["flags"] & U) == 0)
    want = _umis_call(filters, tl, st["rec"][S], pack([st["nm"][i] for i in S]), st["sec"][S], pack([st["bc"][i] for i in S]),
                      pack([st["um"][i] for i in S]), model=model, mode=mode, max_iter=max_iter)
    want = _finish_want(st, S, want, want["order"])
    assert want["barcodes"] == list(dict.fromkeys(st["bc"][i] for i in S))      # cells are numbered by their first survivor
    return want


def _expected_collated(st, filters, tl, model=-1, mode="sort", max_iter=MAX_ITER):
    """the join on the survivors: collate_names with the streamed cells, dedup_umis, drop_groups, the records call"""
    S, cro, labels = _walk(st)
    rec = np.ascontiguousarray(st["rec"][S])
    order, goff, cgo = oarfish_amd.collate_names(pack([st["nm"][i] for i in S]), cro, st["sec"][S], mode=mode)
    dup, _, cell_dups = oarfish_amd.dedup_umis(pack([st["um"][i] for i in S]), order, goff, cgo, flags=rec["flags"])
    order2, goff2, cgo2, cro2 = oarfish_amd.drop_groups(order, goff, cgo, dup)
    ref = oarfish_amd.em_cells_records_sparse(filters, tl, rec[order2], goff2, cgo2, coverage=COVS[model], max_iter=max_iter, conv_thresh=1e-3)
    want = dict(cell_rec_off=cro2, group_off=goff2, cell_group_off=cgo2, kept=ref[4], tables=ref[5], cells=ref[:4], cell_dups=cell_dups)
    want = _finish_want(st, S, want, order2)
    assert want["barcodes"] == labels
    return want


def _expected(collated, *a, **kw):
    return (_expected_collated if collated else _expected_any_order)(*a, **kw)


def _session(batches, filters, tl, collated, model=-1, mode="sort", max_iter=MAX_ITER, push=None, umis=True, **opts):
    with oarfish_amd.CellsStream(len(tl), max_iter=max_iter, conv_thresh=1e-3, coverage=COVS[model], filters=filters, txp_len=tl,
                                 barcodes=True, collated=collated, mode=mode, umis=umis, **opts) as cs:
        if push is not None:
            push(cs)
        else:
            assert [cs.push_batch(*b) for b in batches] == list(range(len(batches)))
        cells = cs.finish()
        out = cs.cells()
        out.update(cells=cells, tables=cs.discard_tables(), info=cs.info())
    return out


def _same_umis(got, want, label):
    _same(got, want, label)
    assert got["cell_dups"].dtype == np.uint64 and np.array_equal(got["cell_dups"], want["cell_dups"]), f"{label}: cell_dups"
    info = got["info"]
    assert info["umi_dup_reads"] == int(want["cell_dups"].sum()) and info["umi_dup_records"] == want["dup_records"], f"{label}: info"
    # records accepted = n_unmapped + n_survivors + UMI_DUP_RECORDS
    assert info["alignments"] == got["n_unmapped"] + len(got["order"]) + info["umi_dup_records"], f"{label}: the record counts"
    assert int(got["cell_rec_off"][-1]) == len(got["order"]) == int(got["group_off"][-1]), f"{label}: positions"


# ---- 1. a hand-built input, every set of at most two cuts -----------------------------------------------------------------
A, B, CC, D = b"AAAA", b"CC", b"ACGT-1", b"G"
#            barcode name     secondary unmapped UMI
INPUT17 = [(A, b"r2", 0, 0, b"ACGT"),      # 0   class ACGT of A: r1 sorts first, so the LATER record survives
           (A, b"r1", 0, 0, b"ACGT"),      # 1
           (A, b"r3", 0, 0, b"ACG"),       # 2   ACG beside ACGT
           (A, b"r4", 0, 0, b""),          # 3   a primary without UMI ...
           (A, b"r4", 1, 0, b"ACG"),       # 4   ... whose secondary carries another read's: r4 takes no part
           (A, GARBAGE, 1, 1, GARBAGE),    # 5   unmapped, inside a cell, with a UMI no survivor may carry
           (A, b"r5", 0, 0, b"ACG"),       # 6   a duplicate of r3
           (B, b"x", 0, 0, b"ACGT"),       # 7   the UMI of another cell: kept
           (B, b"y", 0, 0, P9),            # 8   two UMIs that first differ in the second 8-byte word
           (B, b"z", 0, 0, Q9),            # 9
           (CC, b"p", 0, 0, b"TT"),        # 10  a cell whose reads are all one class
           (CC, b"q", 0, 0, b"TT"),        # 11
           (CC, b"q", 1, 0, b"TT"),        # 12
           (D, b"solo", 0, 0, b"TT"),      # 13  a single-record cell
           (A, b"r9", 0, 0, b"ACGT"),      # 14  the barcode comes back with the UMIs of its first run
           (A, b"r0", 0, 0, b"ACG"),       # 15
           (b"", GARBAGE, 0, 1, b"")]      # 16
N17 = len(INPUT17)


def _stream17():
    rng = np.random.default_rng(17)
    rec = np.zeros(N17, dtype=ALN_RECORD)
    for i, row in enumerate(INPUT17):
        rec[i] = (int(rng.integers(0, EDGE_T)), 10, 1500, 1400, 1000 - int(rng.integers(0, 30)), 1500, U if row[3] else _lib.REC_HAS_SCORE, 0)
    return _ustream(rec, *[[row[k] for row in INPUT17] for k in (0, 1, 2, 4)])


def _wants17():
    st, tl = _stream17(), np.full(EDGE_T, 2000, dtype=np.uint64)
    return st, tl, {c: _expected(c, st, EDGE_FILTERS, tl, max_iter=20) for c in FORMS}


def test_the_hand_built_input_is_what_the_issue_asks_for():
    st, _, wants = _wants17()
    assert 16 <= N17 <= 20 and st["um"][5] == b"\x00\xff" and (st["rec"]["flags"][5] & U) and st["bc"][4] == st["bc"][6] == A
    assert P9[:8] == Q9[:8] and P9[8] != Q9[8] and len(P9) > 8 and {st["um"][8], st["um"][9]} == {P9, Q9}
    assert st["um"][2] == b"ACG" and st["um"][1] == b"ACGT"                            # ACG beside ACGT
    assert st["um"][3] == b"" and st["sec"][4] == 1 and st["nm"][3] == st["nm"][4] and st["um"][4] == st["um"][2]
    # the any-order form: A is one cell of eight survivors; r0 (15) and r1 (1) sort first and survive the earlier records
    w = wants[False]
    assert w["barcodes"] == [A, B, CC, D] and w["n_unmapped"] == 2
    assert list(w["order64"]) == [15, 1, 3, 4, 7, 8, 9, 10, 13] and list(w["cell_dups"]) == [4, 0, 1, 0]
    assert list(w["cell_rec_off"]) == [0, 4, 7, 8, 9] and list(w["group_off"]) == [0, 1, 2, 4, 5, 6, 7, 8, 9]
    # the collated form: A comes back as a NEW cell with the same UMIs, and nothing is merged
    w = wants[True]
    assert w["barcodes"] == [A, B, CC, D, A] and list(w["cell_dups"]) == [2, 0, 1, 0, 0]
    assert list(w["order64"]) == [1, 2, 3, 4, 7, 8, 9, 10, 13, 15, 14] and list(w["cell_rec_off"]) == [0, 4, 7, 8, 9, 11]
    for w in wants.values():
        order = [int(i) for i in w["order64"]]
        assert 1 in order and 0 not in order            # the survivor of {r2 (0), r1 (1)} is the later record: its name sorts first
        assert 3 in order and 4 in order                # the read with the empty primary UMI takes no part
        assert 7 in order                               # one UMI in two different cells: both kept
        assert 8 in order and 9 in order                # the long UMIs differ
        assert 10 in order and 11 not in order and 12 not in order and 13 in order   # one read left; the single-record cell
        # a survivor and its duplicate are separated by single cuts: they fall into different batches
        assert any(a < c <= b for c in range(1, N17) for a, b in ((0, 1), (10, 11)))


@pytest.mark.parametrize("collated", FORMS)
def test_every_cutting_of_the_hand_built_input_at_up_to_two_positions(collated):
    st, tl = _stream17(), np.full(EDGE_T, 2000, dtype=np.uint64)
    want = _expected(collated, st, EDGE_FILTERS, tl, max_iter=20)
    cuttings = [c for k in (0, 1, 2) for c in itertools.combinations(range(1, N17), k)]
    assert len(cuttings) == 137
    for cuts in cuttings:
        got = _session(_cut(st, [0, *cuts, N17]), EDGE_FILTERS, tl, collated, max_iter=20)
        _same_umis(got, want, f"collated {collated}, cuts {cuts}")


# ---- 2. the interleaved fixture with duplicates, in cycled batch sizes -----------------------------------------------------
def _fixture(aug, collated, mode="sort"):   # noqa: F811
    fx = aug(True)
    key = ("stream", collated, mode)
    if key not in fx["joins"]:
        f, tl, rec, names, sec, bc, umis = fx["args"]
        if mode == "adjacent":   # name-collated inside every cell, the cells' places in the stream as they are: the cut finds the same reads
            order_bc, cro = oarfish_amd.collate_barcodes(bc)
            order_names, _, _ = oarfish_amd.collate_names(gather_names(names, order_bc), cro, np.asarray(sec)[order_bc])
            perm = np.empty(len(rec), dtype=np.int64)
            perm[order_bc.astype(np.int64)] = order_bc[order_names.astype(np.int64)]
            rec, names, sec, bc, umis = rec[perm], gather_names(names, perm), np.asarray(sec)[perm], gather_names(bc, perm), gather_names(umis, perm)
        if collated:        # stably by each barcode's first occurrence: input with UMIs and duplicates for the collated form
            perm = synth.recollate_by_first_barcode(bc)
            assert not np.array_equal(perm, np.arange(len(rec)))
            rec, names, sec, bc, umis = rec[perm], gather_names(names, perm), np.asarray(sec)[perm], gather_names(bc, perm), gather_names(umis, perm)
        (r, b, nm, s, um), = synth.cut_interleaved_records(rec, names, sec, bc, (), unmapped_every=7, umis=umis)
        b, nm, um = _unpack(b), _unpack(nm), _unpack(um)
        for i in np.flatnonzero((r["flags"] & U) != 0):     # bytes no survivor may carry
            b[i], nm[i], um[i] = GARBAGE, GARBAGE, GARBAGE
        st = _ustream(r, b, nm, s, um)
        st["rec"].setflags(write=False)
        fx["joins"][key] = dict(st=st, refs={})
    return fx["joins"][key], fx


def _ref(aug, collated, model, mode):   # noqa: F811
    held, fx = _fixture(aug, collated, mode)
    if (model, mode) not in held["refs"]:
        f, tl = fx["args"][:2]
        ref = _expected(collated, held["st"], f, tl, model, mode)
        assert int(ref["cell_dups"].sum()) > 2000, "nothing is deduplicated"
        assert int((ref["kept"] > 0).sum()) > 0.5 * len(ref["kept"]), "the filter dropped the reads"
        assert {bc: int(d) for bc, d in zip(ref["barcodes"], ref["cell_dups"]) if d} == fx["copies"]   # the generator's copies
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        held["refs"][(model, mode)] = ref
    return held["st"], held["refs"][(model, mode)], fx["args"][0], fx["args"][1]


@pytest.mark.parametrize("mode", ["sort", "adjacent"])
@pytest.mark.parametrize("model", [-1, 1])
@pytest.mark.parametrize("collated", FORMS)
def test_fixture_with_duplicates_in_cycled_batch_sizes(aug, collated, model, mode):   # noqa: F811
    st, want, f, tl = _ref(aug, collated, model, mode)
    batches = _cut(st, _cycled(len(st["rec"])))
    assert {len(b[0]) for b in batches[:-1]} == set(SIZES)
    # the collated form under small budgets: several groups run under later batches, with back-pressure
    opts = dict(group_nnz=2000, max_staged_nnz=3000) if collated else {}
    got = _session(batches, f, tl, collated, model, mode, **opts)
    _same_umis(got, want, f"collated {collated}, model {model}, {mode}")
    assert got["info"]["umi_dup_reads"] > 2000 and got["info"]["alignments"] == len(st["rec"])
    if collated:
        assert got["info"]["groups_before_finish"] > 0 and got["info"]["groups"] > 3
    else:
        assert got["info"]["groups_before_finish"] == 0
        assert got["info"]["arena_bytes"] >= len(want["S"]) * (40 + 8 + 8 + 1 + 4 + 8) + sum(len(st["um"][i]) for i in want["S"])


# ---- 3. every UMI empty: the session without UMIs ---------------------------------------------------------------------------
@pytest.mark.parametrize("collated", FORMS)
def test_all_umis_empty_equal_the_session_without_umis(aug, collated):   # noqa: F811
    st, _, f, tl = _ref(aug, collated, -1, "sort")
    batches = _cut(st, _cycled(len(st["rec"])))
    plain = _session([b[:4] for b in batches], f, tl, collated, umis=False)
    for how in ("none", "empty"):      # umis=None, or a list of empty strings
        got = _session([b[:4] + (None if how == "none" else [b""] * len(b[0]),) for b in batches], f, tl, collated)
        assert "cell_dups" not in plain and not got["cell_dups"].any() and len(got["cell_dups"]) == len(got["barcodes"])
        assert got["info"]["umi_dup_reads"] == 0 and got["info"]["umi_dup_records"] == 0 and plain["info"]["umi_dup_reads"] == 0
        plain.update(order64=plain["order"])
        _same(got, plain, f"collated {collated}, {how}")
        for k in (0, 1):
            assert np.array_equal(got["cells"][k], plain["cells"][k])


# ---- 4. four pushing threads: the tickets give the order ------------------------------------------------------------------
@pytest.mark.parametrize("collated", FORMS)
def test_four_threads_push_and_the_tickets_give_the_order(aug, collated):   # noqa: F811
    st, _, f, tl = _ref(aug, collated, -1, "sort")
    n = min(len(st["rec"]), 6000)
    batches = _cut(st, list(range(0, n, 300)) + [n])
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

    got = _session(None, f, tl, collated, push=push)
    assert sorted(tickets) == list(range(len(batches)))
    by_ticket = [batches[k] for k in np.argsort(tickets)]
    pushed = _ustream(np.concatenate([b[0] for b in by_ticket]), *[sum((list(b[k]) for b in by_ticket), []) for k in (1, 2)],
                      np.concatenate([b[3] for b in by_ticket]), sum((list(b[4]) for b in by_ticket), []))
    _same_umis(got, _expected(collated, pushed, f, tl), f"four threads, collated {collated}")


# ---- 5. errors ----------------------------------------------------------------------------------------------------------------
def _fails(batches, at, collated, code, words):
    """the error comes out of finish (or of a push behind the faulty batch), with these words, and sticks"""
    tl = np.full(EDGE_T, 2000, dtype=np.uint64)
    with oarfish_amd.CellsStream(EDGE_T, max_iter=20, filters=EDGE_FILTERS, txp_len=tl, barcodes=True, collated=collated, umis=True) as cs:
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


@pytest.mark.parametrize("collated", FORMS)
def test_a_0_byte_in_a_survivors_umi_in_the_third_batch(collated):
    st = _stream17()
    st["um"][11], st["um"][12] = b"T\x00T", b"\x00"             # two bad records in the third batch: the smallest index wins
    edges = [0, 5, 9, 14, N17]
    _fails(_cut(st, edges), 2, collated, _lib.OEM_ERR_ARG, ["oem_cells_stream", "ticket 2", "the UMI of record 11 contains a 0 byte"])
    st["nm"][11] = b"q\x00"                                       # on a tie the order is barcode, name, UMI
    _fails(_cut(st, edges), 2, collated, _lib.OEM_ERR_ARG, ["ticket 2", "the name of record 11 contains a 0 byte"])
    # the same bytes in an unmapped record's UMI are no error (record 5 carries them all along)
    st = _stream17()
    st["um"][16] = b"T\x00T"
    want = _expected(collated, st, EDGE_FILTERS, np.full(EDGE_T, 2000, dtype=np.uint64), max_iter=20)
    _same_umis(_session(_cut(st, edges), EDGE_FILTERS, np.full(EDGE_T, 2000, dtype=np.uint64), collated, max_iter=20), want, "unmapped")


def test_a_bad_ref_id_in_a_duplicate_differs_between_the_forms():
    st, tl = _stream17(), np.full(EDGE_T, 2000, dtype=np.uint64)
    st["rec"]["ref_id"][11] = EDGE_T + 3                          # record 11 is a duplicate in both forms: its class keeps p (10)
    edges = [0, 5, 9, 14, N17]
    # the any-order form checks every surviving record of a batch
    _fails(_cut(st, edges), 2, False, _lib.OEM_ERR_ARG, ["ticket 2", "record 11:", f"ref_id {EDGE_T + 3} is not below n_txps"])
    # the collated form looks among the reads that remain: the duplicate's records are never gathered
    got = _session(_cut(st, edges), EDGE_FILTERS, tl, True, max_iter=20)
    assert 11 not in got["order"] and list(got["cell_dups"]) == [2, 0, 1, 0, 0]
    st["rec"]["ref_id"][10] = EDGE_T + 4                          # ... and finds the survivor's
    _fails(_cut(st, edges), 2, True, _lib.OEM_ERR_ARG, ["ticket 2", "record 10:", f"ref_id {EDGE_T + 4} is not below n_txps"])


def test_state_errors_with_a_device():
    L = _lib.lib()
    tl = np.full(EDGE_T, 2000, dtype=np.uint64)
    st = _stream17()
    whole, = _cut(st, [0, N17])
    for collated in FORMS:
        with oarfish_amd.CellsStream(EDGE_T, filters=EDGE_FILTERS, txp_len=tl, barcodes=True, collated=collated, umis=True, max_iter=20) as cs:
            assert L.oem_cells_stream_set_umis(cs._h) == _lib.OEM_ERR_STATE and b"already" in L.oem_last_error()      # a second time
            off = np.zeros(1, dtype=np.uint64)
            assert L.oem_cells_stream_push_barcodes(cs._h, None, 0, None, off.ctypes.data, None, off.ctypes.data, None,
                                                    None) == _lib.OEM_ERR_STATE and b"push_barcodes_umis" in L.oem_last_error()   # the plain push
            assert L.oem_cells_stream_umis_copy(cs._h, None) == _lib.OEM_ERR_STATE                                    # before finish
            cs.push_batch(*whole)
            cs.finish()
            assert L.oem_cells_stream_set_umis(cs._h) == _lib.OEM_ERR_STATE                                           # after finish
            assert L.oem_cells_stream_umis_copy(cs._h, None) == _lib.OEM_ERR_ARG
        with oarfish_amd.CellsStream(EDGE_T, filters=EDGE_FILTERS, txp_len=tl, barcodes=True, collated=collated, max_iter=20) as cs:
            off = np.zeros(1, dtype=np.uint64)
            assert L.oem_cells_stream_push_barcodes_umis(cs._h, None, 0, None, off.ctypes.data, None, off.ctypes.data, None, None,
                                                         off.ctypes.data, None) == _lib.OEM_ERR_STATE                  # no UMI session
            with pytest.raises(ValueError, match="UMI session"):
                cs.push_batch(*whole)
            cs.push_batch(*whole[:4])
            assert L.oem_cells_stream_set_umis(cs._h) == _lib.OEM_ERR_STATE and b"pushed" in L.oem_last_error()       # after a push
            cs.finish()
            assert L.oem_cells_stream_umis_copy(cs._h, np.zeros(8, dtype=np.uint64).ctypes.data) == _lib.OEM_ERR_STATE
            assert cs.info()["umi_dup_reads"] == 0 and cs.info()["umi_dup_records"] == 0
    with oarfish_amd.CellsStream(EDGE_T, filters=EDGE_FILTERS, txp_len=tl) as cs:                                      # a records session
        assert L.oem_cells_stream_set_umis(cs._h) == _lib.OEM_ERR_STATE and b"barcoded" in L.oem_last_error()
        assert L.oem_cells_stream_umis_copy(cs._h, None) == _lib.OEM_ERR_STATE
    with oarfish_amd.CellsStream(EDGE_T) as cs:                                                                        # a plain session
        assert L.oem_cells_stream_set_umis(cs._h) == _lib.OEM_ERR_STATE
    # an argument error rejects the batch only and uses no ticket
    with oarfish_amd.CellsStream(EDGE_T, filters=EDGE_FILTERS, txp_len=tl, barcodes=True, umis=True, max_iter=20) as cs:
        with pytest.raises(ValueError, match="umis"):
            cs.push_batch(*whole[:4], whole[4][:-1])
        blob = np.frombuffer(b"ACGT" * N17, dtype=np.uint8)
        with pytest.raises(oarfish_amd.OemError) as ei:
            cs.push_batch(*whole[:4], (blob, np.arange(1, N17 + 2, dtype=np.uint64)))
        assert ei.value.code == _lib.OEM_ERR_ARG and "umi_off must start at 0" in str(ei.value)
        assert cs.push_batch(*whole) == 0
        cs.finish()
        assert list(cs.cells()["cell_dups"]) == [2, 0, 1, 0, 0]


# ---- 6. the host loop -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("collated", FORMS)
@pytest.mark.parametrize("case", ["big_score", "zero_denom"])
def test_host_loop_fallbacks_on_input_with_duplicates(aug, case, collated):   # noqa: F811
    full, _, f, tl = _ref(aug, collated, -1, "sort")
    n = 3000
    st = _ustream(full["rec"][:n].copy(), full["bc"][:n], full["nm"][:n], full["sec"][:n], full["um"][:n])
    filters = dict(f)
    if case == "big_score":
        i = int(np.flatnonzero((st["rec"]["flags"] & U) == 0)[1400])
        st["rec"]["score"][i] = 2 ** 24 + 1
        st["rec"]["flags"][i] |= _lib.REC_HAS_SCORE
    else:
        filters["score_prob_denom"] = 0.0
    want = _expected(collated, st, filters, tl)
    assert int(want["cell_dups"].sum()) > 20
    got = _session(_cut(st, _cycled(n, [1, 64, 257, 100])), filters, tl, collated, group_cells=3)
    _same_umis(got, want, f"{case}, collated {collated}")
    assert got["info"]["groups"] >= len(want["barcodes"]) // 3


# ---- 7. the driver --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("collated", FORMS)
def test_the_driver_writes_the_files_of_the_expected_side(aug, tmp_path, collated):   # noqa: F811
    import json
    st, want, f, tl = _ref(aug, collated, 1, "sort")
    names = [f"t{i}" for i in range(T)]
    args = SingleCellArgs(output=str(tmp_path / "stream" / "out"), max_em_iter=MAX_ITER, model_coverage="binomial", collated=collated, umis=True)
    got = quantify_single_cell_from_record_batches(f, names, tl, _cut(st, _cycled(len(st["rec"]))), args)
    assert got[4]["barcodes"] == want["barcodes"] and np.array_equal(got[4]["cell_dups"], want["cell_dups"])
    ref_out = str(tmp_path / "expected" / "out")
    info = {"output": args.output, "single_cell": True, "em_max_iter": MAX_ITER, "em_convergence_thresh": 1e-3, "threads": 3,
            "filter_options": {"model_coverage": True}, "umi_dedup": True, "umi_duplicate_reads": int(want["cell_dups"].sum())}
    indptr, cols, vals, _ = want["cells"]
    writers.write_single_cell_output_device(ref_out, info, names, [b.decode("latin-1") for b in want["barcodes"]], len(want["barcodes"]),
                                            indptr, cols, vals)
    for ext in (".count.mtx", ".features.txt", ".barcodes.txt", ".meta_info.json"):
        a, b = open(args.output + ext, "rb").read(), open(ref_out + ext, "rb").read()
        assert a == b and len(a) > 0, ext
    meta = json.load(open(args.output + ".meta_info.json"))
    assert meta["umi_dedup"] is True and meta["umi_duplicate_reads"] > 2000
    # without umis the driver is unchanged: 4-tuples, no new keys
    plain = SingleCellArgs(output=str(tmp_path / "plain" / "out"), max_em_iter=MAX_ITER, collated=collated)
    res = quantify_single_cell_from_record_batches(f, names, tl, [b[:4] for b in _cut(st, _cycled(len(st["rec"])))], plain)
    meta = json.load(open(plain.output + ".meta_info.json"))
    assert "umi_dedup" not in meta and "umi_duplicate_reads" not in meta and "cell_dups" not in res[4]
