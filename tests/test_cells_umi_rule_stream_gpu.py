"""GPU tests of the UMI rule in the two barcoded sessions (oem_cells_stream_set_umi_rule / _umi_rule_copy): gene-aware keys
and one-mismatch correction in every group's deduplication.

The any-order form is held to the rule one call (oem_em_run_cells_records_umis_rule_sparse) on the surviving records; the
collated form, where a barcode that comes back is a new cell, to the join: oem_collate_names with the streamed cells,
oem_dedup_umis_rule with the survivors' ref_ids, the duplicates dropped, oem_em_run_cells_records_sparse.  The comparison
is tests/test_cells_umis_stream_gpu.py's (_same_umis) plus cell_corrected and info()["umi_corrected_reads"].  The expected
side never comes from a session."""
import ctypes as C
import itertools
import json
import threading

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth, writers
from oarfish_amd.builder import ALN_RECORD
from oarfish_amd.em import UmiRuleC, gather_names
from oarfish_amd.single_cell import SingleCellArgs, quantify_single_cell_from_record_batches
from tests.test_cells_barcodes_stream_gpu import EDGE_FILTERS, GARBAGE, SIZES, U, _cycled, _unpack, _walk
from tests.test_cells_records_gpu import COVS
from tests.test_cells_records_names_gpu import pack
from tests.test_cells_umis_stream_gpu import FORMS, _cut, _finish_want, _same_umis, _session, _ustream
from tests.test_collate_gpu import MAX_ITER, T
from tests.test_dedup_umis_gpu import aug, base, inter   # noqa: F401  (fixtures)
from tests.test_dedup_umis_rule import COMBOS
from tests.test_dedup_umis_rule_gpu import _one_call as _rule_call, erred   # noqa: F401  (erred: a fixture)
from tests.test_gene_counts import same as same_counts, walk as gene_walk

pytestmark = pytest.mark.gpu


# ---- the two expected sides and the comparison ------------------------------------------------------------------------------
def _expected_any_order(st, filters, tl, gene_of, correct, model=-1, mode="sort", max_iter=MAX_ITER):
    """the rule one call on the survivors"""
    S = np.flatnonzero((st["rec"]["flags"] & U) == 0)
    want = _rule_call(filters, tl, st["rec"][S], pack([st["nm"][i] for i in S]), st["sec"][S], pack([st["bc"][i] for i in S]),
                      pack([st["um"][i] for i in S]), gene_of, correct, model=model, mode=mode, max_iter=max_iter)
    want = _finish_want(st, S, want, want["order"])
    assert want["barcodes"] == list(dict.fromkeys(st["bc"][i] for i in S))
    return want


def _expected_collated(st, filters, tl, gene_of, correct, model=-1, mode="sort", max_iter=MAX_ITER):
    """the join on the survivors: collate_names with the streamed cells, dedup_umis_rule, drop_groups, the records call"""
    S, cro, labels = _walk(st)
    rec = np.ascontiguousarray(st["rec"][S])
    order, goff, cgo = oarfish_amd.collate_names(pack([st["nm"][i] for i in S]), cro, st["sec"][S], mode=mode)
    dup, _, cell_dups, cell_corrected = oarfish_amd.dedup_umis_rule(pack([st["um"][i] for i in S]), order, goff, cgo, flags=rec["flags"],
                                                                    ref_id=rec["ref_id"], gene_of=gene_of, correct=correct)
    order2, goff2, cgo2, cro2 = oarfish_amd.drop_groups(order, goff, cgo, dup)
    ref = oarfish_amd.em_cells_records_sparse(filters, tl, rec[order2], goff2, cgo2, coverage=COVS[model], max_iter=max_iter, conv_thresh=1e-3)
    want = dict(cell_rec_off=cro2, group_off=goff2, cell_group_off=cgo2, kept=ref[4], tables=ref[5], cells=ref[:4], cell_dups=cell_dups,
                cell_corrected=cell_corrected)
    want = _finish_want(st, S, want, order2)
    assert want["barcodes"] == labels
    return want


def _expected(collated, *a, **kw):
    want = (_expected_collated if collated else _expected_any_order)(*a, **kw)
    want["cell_corrected"] = np.asarray(want["cell_corrected"], dtype=np.uint64)
    return want


def _same_rule(got, want, label, correct=True):
    _same_umis(got, want, label)
    if correct:
        assert got["cell_corrected"].dtype == np.uint64 and np.array_equal(got["cell_corrected"], want["cell_corrected"]), f"{label}: cell_corrected"
        assert got["info"]["umi_corrected_reads"] == int(want["cell_corrected"].sum()), f"{label}: umi_corrected_reads"
    else:
        assert "cell_corrected" not in got and got["info"]["umi_corrected_reads"] == 0 and not want["cell_corrected"].any(), label


# ---- 1. a hand-built input: 8 transcripts in 4 genes, every set of at most two cuts -------------------------------------------
T8 = 8
TL8 = np.full(T8, 2000, dtype=np.uint64)
GENE_OF8 = [0, 0, 1, 1, 2, 2, 3, 3]
A, B = b"AAAA", b"CC"
#            barcode name  secondary unmapped UMI    transcript
INPUT21 = [(A, b"a1", 0, 0, b"AAAA", 0),       # 0   one UMI in two genes of one cell: two molecules with gene keys, one without
           (A, b"a2", 0, 0, b"AAAA", 2),       # 1
           (A, b"b0", 0, 0, b"CCCG", 4),       # 2   2 against 1: the erred read sorts first -- a corrected survivor
           (A, b"b1", 0, 0, b"CCCC", 4),       # 3
           (A, b"b2", 0, 0, b"CCCC", 5),       # 4   (another transcript of the gene)
           (A, b"c1", 0, 0, b"GGGG", 6),       # 5   a chain 3 - 2 - 1: GGTT -> GGGT -> GGGG
           (A, b"c2", 0, 0, b"GGGG", 6),       # 6
           (A, b"c3", 0, 0, b"GGGG", 7),       # 7
           (A, b"c4", 0, 0, b"GGGT", 6),       # 8
           (A, GARBAGE, 1, 1, GARBAGE, 0),     # 9   an unmapped record inside a read
           (A, b"c4", 1, 0, b"GGGT", 6),       # 10
           (A, b"c5", 0, 0, b"GGGT", 6),       # 11
           (A, b"c6", 0, 0, b"GGTT", 7),       # 12
           (A, b"d1", 0, 0, b"", 1),           # 13  a read without UMI
           (B, b"t1", 0, 0, b"TTAA", 1),       # 14  a tie: TTAC is one mismatch from TTAA and from TTCC, two reads each
           (B, b"t2", 0, 0, b"TTAA", 0),       # 15
           (B, b"t3", 0, 0, b"TTCC", 1),       # 16
           (B, b"t4", 0, 0, b"TTCC", 1),       # 17
           (B, b"t5", 0, 0, b"TTAC", 0),       # 18
           (B, b"n1", 0, 0, b"CCCA", 4),       # 19  a neighbour of A's CCCC in another cell
           (A, b"z1", 0, 0, b"CCCT", 4)]       # 20  the barcode comes back, one mismatch from its first run's CCCC
N21 = len(INPUT21)


def _stream21():
    rng = np.random.default_rng(21)
    rec = np.zeros(N21, dtype=ALN_RECORD)
    for i, row in enumerate(INPUT21):
        rec[i] = (row[5], 10, 1500, 1400, 1000 - int(rng.integers(0, 30)), 1500, U if row[3] else _lib.REC_HAS_SCORE, 0)
    return _ustream(rec, *[[row[k] for row in INPUT21] for k in (0, 1, 2, 4)])


def _rule(genes, correct):
    return dict(gene_of=GENE_OF8 if genes else None, umi_correct=bool(correct))


def test_the_hand_built_input_holds_what_it_is_built_for():
    """On the expected sides alone."""
    st = _stream21()
    w = {(c, g, k): _expected(c, st, EDGE_FILTERS, TL8, GENE_OF8 if g else None, k, max_iter=20) for c in FORMS for g, k in COMBOS}
    order = lambda key: [int(i) for i in w[key]["order64"]]   # noqa: E731
    for c in FORMS:
        assert 1 in order((c, True, False)) and 1 not in order((c, False, False))          # one UMI in two genes
        assert 2 in order((c, True, True)) and 3 not in order((c, True, True)) and 3 in order((c, True, False))   # the corrected survivor
        assert [i for i in (5, 6, 7, 8, 10, 11, 12) if i in order((c, True, True))] == [5]  # the chain ends in one molecule
        assert 12 in order((c, True, False)) and 8 in order((c, True, False))
        assert 14 in order((c, True, True)) and 16 in order((c, True, True)) and 18 not in order((c, True, True))   # the tie goes to TTAA ...
        assert 19 in order((c, True, True))                                                # the neighbour in another cell stays
        assert 13 in order((c, True, True)) and 9 not in order((c, True, True))            # no UMI: no part; unmapped: skipped
        assert w[(c, True, True)]["n_unmapped"] == 1
    # the barcode that comes back: the any-order form corrects across the two runs, the collated form does not
    assert w[(False, True, True)]["barcodes"] == [A, B] and list(w[(False, True, True)]["cell_corrected"]) == [5, 1]
    assert w[(True, True, True)]["barcodes"] == [A, B, A] and list(w[(True, True, True)]["cell_corrected"]) == [4, 1, 0]
    assert 20 not in order((False, True, True)) and 20 in order((True, True, True))
    assert list(w[(False, True, True)]["cell_dups"]) == [8, 3] and list(w[(True, True, True)]["cell_dups"]) == [7, 3, 0]
    # without genes a cell is one segment: AAAA is one molecule
    assert list(w[(True, False, True)]["cell_dups"]) == [8, 3, 0]


@pytest.mark.parametrize("genes,correct", COMBOS)
@pytest.mark.parametrize("collated", FORMS)
def test_every_cutting_of_the_hand_built_input_at_up_to_two_positions(collated, genes, correct):
    st = _stream21()
    want = _expected(collated, st, EDGE_FILTERS, TL8, GENE_OF8 if genes else None, correct, max_iter=20)
    cuttings = [c for k in (0, 1, 2) for c in itertools.combinations(range(1, N21), k)]
    assert len(cuttings) == 211
    for cuts in cuttings:
        got = _session(_cut(st, [0, *cuts, N21]), EDGE_FILTERS, TL8, collated, max_iter=20, **_rule(genes, correct))
        _same_rule(got, want, f"collated {collated}, genes {genes}, correct {correct}, cuts {cuts}", correct)


# ---- 2. the erred fixture of tests/test_dedup_umis_rule_gpu.py, cut into batches ------------------------------------------------
def _plant_collisions(st, gene_of, per_cell=10):
    """The fixture's UMIs are long enough that no two molecules of different genes share one in a cell, so its gene-keyed
    result equals the gene-less one.  This gives pairs of reads of one cell whose records share no gene the same UMI, in
    all their records: one molecule without gene keys, two with them.  Returns the pairs planted."""
    reads = {}
    for i in np.flatnonzero((st["rec"]["flags"] & U) == 0):
        reads.setdefault(st["bc"][i], {}).setdefault(st["nm"][i], []).append(int(i))
    planted = 0
    for cell in reads.values():
        rs = [r for r in cell.values() if st["um"][r[0]]]
        done = 0
        for a, b in zip(rs[0::2], rs[1::2]):
            if done == per_cell:
                break
            if {int(gene_of[st["rec"]["ref_id"][i]]) for i in a} & {int(gene_of[st["rec"]["ref_id"][i]]) for i in b}:
                continue
            for i in a + b:
                st["um"][i] = st["um"][a[0]]
            done += 1
        planted += done
    return planted


@pytest.fixture(scope="module")
def streams(erred):   # noqa: F811
    """(collated, mode) -> the erred input as a stream for that form, with its annotation and the expected sides by rule."""
    cache = {}

    def get(collated, mode="sort"):
        if (collated, mode) not in cache:
            fx = erred(True)
            f, tl, rec, names, sec, bc, umis = fx["args"]
            if mode == "adjacent":   # name-collated inside every cell, the cells' places in the stream as they are
                order_bc, cro = oarfish_amd.collate_barcodes(bc)
                order_names, _, _ = oarfish_amd.collate_names(gather_names(names, order_bc), cro, np.asarray(sec)[order_bc])
                perm = np.empty(len(rec), dtype=np.int64)
                perm[order_bc.astype(np.int64)] = order_bc[order_names.astype(np.int64)]
                rec, names, sec, bc, umis = rec[perm], gather_names(names, perm), np.asarray(sec)[perm], gather_names(bc, perm), gather_names(umis, perm)
            if collated:
                perm = synth.recollate_by_first_barcode(bc)
                rec, names, sec, bc, umis = rec[perm], gather_names(names, perm), np.asarray(sec)[perm], gather_names(bc, perm), gather_names(umis, perm)
            (r, b, nm, s, um), = synth.cut_interleaved_records(rec, names, sec, bc, (), unmapped_every=7, umis=umis)
            b, nm, um = _unpack(b), _unpack(nm), _unpack(um)
            for i in np.flatnonzero((r["flags"] & U) != 0):     # bytes no survivor may carry
                b[i], nm[i], um[i] = GARBAGE, GARBAGE, GARBAGE
            st = _ustream(r, b, nm, s, um)
            assert _plant_collisions(st, fx["gene_of"]) >= 50
            st["rec"].setflags(write=False)
            cache[(collated, mode)] = dict(st=st, f=f, tl=tl, gene_of=fx["gene_of"], refs={})
        return cache[(collated, mode)]
    return get


def _ref(held, collated, genes=True, correct=True, model=-1, mode="sort"):
    key = (genes, correct, model)
    if key not in held["refs"]:
        held["refs"][key] = _expected(collated, held["st"], held["f"], held["tl"], held["gene_of"] if genes else None, correct, model, mode)
    return held["refs"][key]


def _exercised(held, collated, model=-1, mode="sort"):
    """The bar of test_the_one_call_equals_the_join, on the expected side only: the rule corrects, merges more than the exact
    rule, and its gene keys matter."""
    want = _ref(held, collated, True, True, model, mode)
    assert int(want["cell_corrected"].sum()) > 100, "nothing is corrected"
    assert int(want["cell_dups"].sum()) > int(_ref(held, collated, True, False, model, mode)["cell_dups"].sum()), "the correction merged nothing"
    less = _ref(held, collated, False, True, model, mode)
    assert not (np.array_equal(want["cell_dups"], less["cell_dups"]) and np.array_equal(want["order64"], less["order64"])), "the genes change nothing"
    return want


@pytest.mark.parametrize("mode", ["sort", "adjacent"])
@pytest.mark.parametrize("model", [-1, 1])
@pytest.mark.parametrize("collated", FORMS)
def test_erred_fixture_in_cycled_batch_sizes(streams, collated, model, mode):
    held = streams(collated, mode)
    want = _exercised(held, collated, model, mode)
    st = held["st"]
    batches = _cut(st, _cycled(len(st["rec"])))
    assert {len(b[0]) for b in batches[:-1]} == set(SIZES)
    opts = dict(group_nnz=2000, max_staged_nnz=3000) if collated else {}
    got = _session(batches, held["f"], held["tl"], collated, model, mode, gene_of=held["gene_of"], umi_correct=True, **opts)
    _same_rule(got, want, f"collated {collated}, model {model}, {mode}")
    assert got["info"]["alignments"] == len(st["rec"])


@pytest.mark.parametrize("genes,correct", COMBOS[1:3])
@pytest.mark.parametrize("collated", FORMS)
def test_erred_fixture_under_the_other_rules(streams, collated, genes, correct):
    held = streams(collated)
    _exercised(held, collated)
    st = held["st"]
    got = _session(_cut(st, _cycled(len(st["rec"]))), held["f"], held["tl"], collated, gene_of=held["gene_of"] if genes else None,
                   umi_correct=correct)
    _same_rule(got, _ref(held, collated, genes, correct), f"collated {collated}, genes {genes}, correct {correct}", correct)


@pytest.mark.parametrize("collated", FORMS)
def test_the_rule_in_many_groups(streams, collated):
    """group_cells = 1 and a small group_nnz: every cell is a group of its own, each with its own dedup_mark."""
    held = streams(collated)
    want = _exercised(held, collated)
    st = held["st"]
    got = _session(_cut(st, _cycled(len(st["rec"]))), held["f"], held["tl"], collated, gene_of=held["gene_of"], umi_correct=True,
                   group_cells=1, group_nnz=500)
    _same_rule(got, want, f"many groups, collated {collated}")
    assert got["info"]["groups"] == len(want["barcodes"]) > 3


def test_four_threads_push_and_the_tickets_give_the_order(streams):
    held = streams(True)
    _exercised(held, True)
    st, f, tl = held["st"], held["f"], held["tl"]
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

    got = _session(None, f, tl, True, push=push, gene_of=held["gene_of"], umi_correct=True)
    assert sorted(tickets) == list(range(len(batches)))
    by_ticket = [batches[k] for k in np.argsort(tickets)]
    pushed = _ustream(np.concatenate([b[0] for b in by_ticket]), *[sum((list(b[k]) for b in by_ticket), []) for k in (1, 2)],
                      np.concatenate([b[3] for b in by_ticket]), sum((list(b[4]) for b in by_ticket), []))
    _same_rule(got, _expected(True, pushed, f, tl, held["gene_of"], True), "four threads")


# ---- 3. the empty rule, the errors ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("collated", FORMS)
def test_the_empty_rule_is_the_session_without_one(collated):
    """(NULL gene_of, correct 0) through oem_cells_stream_set_umi_rule: accepted, and exactly the session without the call."""
    st = _stream21()
    batches = _cut(st, [0, 5, 9, 14, N21])
    plain = _session(batches, EDGE_FILTERS, TL8, collated, max_iter=20)
    L = _lib.lib()
    rule = UmiRuleC(None, 0, 0)

    def push(cs):
        assert L.oem_cells_stream_set_umi_rule(cs._h, C.addressof(rule)) == _lib.OEM_OK, L.oem_last_error()
        assert L.oem_cells_stream_set_umi_rule(cs._h, C.addressof(rule)) == _lib.OEM_ERR_STATE and b"already" in L.oem_last_error()
        for b in batches:
            cs.push_batch(*b)

    got = _session(None, EDGE_FILTERS, TL8, collated, max_iter=20, push=push)
    assert "cell_corrected" not in got and got["info"]["umi_corrected_reads"] == 0
    assert all(got["info"][k] == plain["info"][k] for k in ("umi_dup_reads", "umi_dup_records", "alignments", "cells"))
    for k in ("cell_rec_off", "order", "group_off", "cell_group_off", "kept", "cell_dups"):
        assert np.array_equal(got[k], plain[k]), k
    assert got["barcodes"] == plain["barcodes"] and got["tables"] == plain["tables"]
    for k in (0, 1):
        assert np.array_equal(got["cells"][k], plain["cells"][k])
    assert np.array_equal(got["cells"][2].view(np.uint32), plain["cells"][2].view(np.uint32))


def _fails(batches, at, collated, words, **rule):
    """the error comes out of finish (or of a push behind the faulty batch), with these words, and sticks"""
    with oarfish_amd.CellsStream(T8, max_iter=20, filters=EDGE_FILTERS, txp_len=TL8, barcodes=True, collated=collated, umis=True, **rule) as cs:
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
        with pytest.raises(oarfish_amd.OemError) as again:
            cs.push_batch(*batches[0])
        errors.append(again.value)
        for e in errors:
            assert e.code == _lib.OEM_ERR_ARG and all(w in str(e) for w in words), str(e)
        assert str(errors[0]) == str(errors[-1])


def test_a_bad_ref_id_at_a_participating_head():
    """Record 11 (c5) is a duplicate under every rule: its records are never gathered, so in the collated form only the
    rule's gene lookup meets its ref_id -- and words the error as the filter would, with the ticket and the stream index."""
    st = _stream21()
    st["rec"]["ref_id"][11] = T8 + 3
    edges = [0, 5, 9, 14, N21]
    words = ["oem_cells_stream: ticket 2: record 11: ref_id 11 is not below n_txps"]
    _fails(_cut(st, edges), 2, True, words, **_rule(True, True))
    _fails(_cut(st, edges), 2, True, words, **_rule(True, False))
    # without gene keys no ref_id is read at a head, and the duplicate's records never reach the filter
    got = _session(_cut(st, edges), EDGE_FILTERS, TL8, True, max_iter=20, **_rule(False, True))
    assert 11 not in got["order"]
    # the any-order form rejects the record with its batch, as it does without a rule
    _fails(_cut(st, edges), 2, False, ["ticket 2", "record 11:", f"ref_id {T8 + 3} is not below n_txps"], **_rule(True, True))
    # a fresh session afterwards gives the right result
    st = _stream21()
    for collated in FORMS:
        want = _expected(collated, st, EDGE_FILTERS, TL8, GENE_OF8, True, max_iter=20)
        _same_rule(_session(_cut(st, edges), EDGE_FILTERS, TL8, collated, max_iter=20, **_rule(True, True)), want, f"after the error, {collated}")


def test_state_and_argument_errors_with_a_device():
    L = _lib.lib()
    st = _stream21()
    whole, = _cut(st, [0, N21])
    gene = np.array(GENE_OF8, dtype=np.uint32)
    rule = lambda g=gene, n=T8, c=1: UmiRuleC(None if g is None else g.ctypes.data, n, c)   # noqa: E731
    set_rule = lambda cs, r: L.oem_cells_stream_set_umi_rule(cs._h, None if r is None else C.addressof(r))   # noqa: E731
    out = np.zeros(8, dtype=np.uint64)
    for collated in FORMS:
        with oarfish_amd.CellsStream(T8, filters=EDGE_FILTERS, txp_len=TL8, barcodes=True, collated=collated, umis=True, max_iter=20) as cs:
            for bad, words in ((None, b"rule is NULL"), (rule(c=2), b"neither 0 nor 1"), (rule(n=0), b"n_txps is 0"),
                               (rule(n=T8 - 1), b"not the session's n_txps = 8")):
                assert set_rule(cs, bad) == _lib.OEM_ERR_ARG and words in L.oem_last_error(), L.oem_last_error()
            assert L.oem_cells_stream_umi_rule_copy(cs._h, out.ctypes.data) == _lib.OEM_ERR_STATE                    # no rule yet
            assert set_rule(cs, rule()) == _lib.OEM_OK
            assert set_rule(cs, rule()) == _lib.OEM_ERR_STATE and b"already" in L.oem_last_error()                    # once
            assert L.oem_cells_stream_umi_rule_copy(cs._h, out.ctypes.data) == _lib.OEM_ERR_STATE                    # before finish
            gene[:] = 0                                                                                              # (gene_of was copied)
            cs.push_batch(*whole)
            cs.finish()
            gene[:] = GENE_OF8
            assert set_rule(cs, rule()) == _lib.OEM_ERR_STATE                                                         # after finish
            assert L.oem_cells_stream_umi_rule_copy(cs._h, None) == _lib.OEM_ERR_ARG
            n_cells = len(cs.cells()["barcodes"])
            assert L.oem_cells_stream_umi_rule_copy(cs._h, out.ctypes.data) == _lib.OEM_OK
            want = _expected(collated, st, EDGE_FILTERS, TL8, GENE_OF8, True, max_iter=20)
            assert list(out[:n_cells]) == list(want["cell_corrected"])
        with oarfish_amd.CellsStream(T8, filters=EDGE_FILTERS, txp_len=TL8, barcodes=True, collated=collated, umis=True, max_iter=20) as cs:
            cs.push_batch(*whole)
            assert set_rule(cs, rule()) == _lib.OEM_ERR_STATE and b"pushed" in L.oem_last_error()                     # after a push
            cs.finish()
            assert L.oem_cells_stream_umi_rule_copy(cs._h, out.ctypes.data) == _lib.OEM_ERR_STATE                    # a session without a rule
            assert cs.info()["umi_corrected_reads"] == 0
        with oarfish_amd.CellsStream(T8, filters=EDGE_FILTERS, txp_len=TL8, barcodes=True, collated=collated, umis=True, gene_of=GENE_OF8,
                                     max_iter=20) as cs:
            cs.push_batch(*whole)
            cs.finish()
            assert L.oem_cells_stream_umi_rule_copy(cs._h, out.ctypes.data) == _lib.OEM_ERR_STATE                    # a rule without correct
            assert "cell_corrected" not in cs.cells()
        with oarfish_amd.CellsStream(T8, filters=EDGE_FILTERS, txp_len=TL8, barcodes=True, collated=collated, max_iter=20) as cs:
            assert set_rule(cs, rule()) == _lib.OEM_ERR_STATE and b"UMI session" in L.oem_last_error()                # before set_umis
    with oarfish_amd.CellsStream(T8, filters=EDGE_FILTERS, txp_len=TL8) as cs:                                        # a records session
        assert set_rule(cs, rule()) == _lib.OEM_ERR_STATE
        assert L.oem_cells_stream_umi_rule_copy(cs._h, out.ctypes.data) == _lib.OEM_ERR_STATE
    with oarfish_amd.CellsStream(T8) as cs:                                                                           # a plain session
        assert set_rule(cs, rule()) == _lib.OEM_ERR_STATE


# ---- 4. the driver ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("collated", FORMS)
def test_the_driver_writes_six_files(streams, tmp_path, collated):
    held = streams(collated)
    want = _exercised(held, collated, 1)
    st, f, tl, gene_of = held["st"], held["f"], held["tl"], held["gene_of"]
    n_genes = int(np.max(gene_of)) + 1
    names, genes = [f"t{i}" for i in range(T)], [f"gene{g}" for g in range(n_genes)]
    batches = _cut(st, _cycled(len(st["rec"])))
    args = SingleCellArgs(output=str(tmp_path / "stream" / "out"), max_em_iter=MAX_ITER, model_coverage="binomial", collated=collated, umis=True,
                          gene_of=gene_of, gene_names=genes, umi_correct=True, gene_counts=True)
    got = quantify_single_cell_from_record_batches(f, names, tl, batches, args)
    assert got[4]["barcodes"] == want["barcodes"] and np.array_equal(got[4]["cell_dups"], want["cell_dups"])
    assert np.array_equal(got[4]["cell_corrected"], want["cell_corrected"])
    # .count.mtx and the side files are the session's; .gene_count.mtx is this file's walk over the session's matrix
    labels = [b.decode("latin-1") for b in want["barcodes"]]
    session_out = str(tmp_path / "session" / "out")
    writers.write_single_cell_output_device(session_out, {}, names, labels, len(labels), *got[:3])
    for ext in (".count.mtx", ".features.txt", ".barcodes.txt"):
        a, b = open(args.output + ext, "rb").read(), open(session_out + ext, "rb").read()
        assert a == b and len(a) > 0, ext
    assert np.array_equal(got[0], want["cells"][0]) and np.array_equal(got[1], want["cells"][1])
    walked = gene_walk(got[0], got[1], got[2], gene_of)
    assert same_counts(got[4]["gene_counts"], walked) and len(walked[1]) < len(got[1])
    walk_out = str(tmp_path / "walk" / "out")
    writers.write_single_cell_output(walk_out, {}, genes, None, len(labels), *writers.csr_triplets(*walked))
    assert open(args.output + ".gene_count.mtx", "rb").read() == open(walk_out + ".count.mtx", "rb").read()
    assert open(args.output + ".gene_features.txt").read() == "".join(g + "\n" for g in genes)
    meta = json.load(open(args.output + ".meta_info.json"))
    assert meta["umi_dedup"] is True and meta["umi_gene_keys"] is True and meta["umi_correct"] is True
    assert meta["umi_corrected_reads"] == int(want["cell_corrected"].sum()) > 100 and meta["umi_duplicate_reads"] == int(want["cell_dups"].sum())
    assert meta["gene_counts"] is True and meta["n_genes"] == n_genes
    import os
    assert sorted(os.listdir(tmp_path / "stream")) == sorted("out" + e for e in (".count.mtx", ".features.txt", ".barcodes.txt", ".meta_info.json",
                                                                                 ".gene_count.mtx", ".gene_features.txt"))
    # with the four fields at their defaults: today's four files, byte for byte, and today's return value
    plain = SingleCellArgs(output=str(tmp_path / "plain" / "out"), max_em_iter=MAX_ITER, collated=collated, umis=True)
    res = quantify_single_cell_from_record_batches(f, names, tl, batches, plain)
    exact = _ref(held, collated, False, False)
    info = {"output": plain.output, "single_cell": True, "em_max_iter": MAX_ITER, "em_convergence_thresh": 1e-3, "threads": 3,
            "filter_options": {"model_coverage": False}, "umi_dedup": True, "umi_duplicate_reads": int(exact["cell_dups"].sum())}
    ref_out = str(tmp_path / "expected" / "out")
    writers.write_single_cell_output_device(ref_out, info, names, [b.decode("latin-1") for b in exact["barcodes"]], len(exact["barcodes"]),
                                            *res[:3])
    assert sorted(os.listdir(tmp_path / "plain")) == sorted("out" + e for e in (".count.mtx", ".features.txt", ".barcodes.txt", ".meta_info.json"))
    for ext in (".count.mtx", ".features.txt", ".barcodes.txt", ".meta_info.json"):
        assert open(plain.output + ext, "rb").read() == open(ref_out + ext, "rb").read(), ext
    assert np.array_equal(res[1], exact["cells"][1]) and np.array_equal(res[4]["cell_dups"], exact["cell_dups"])
    assert "cell_corrected" not in res[4] and "gene_counts" not in res[4]
    # gene counts alone, on a session without UMIs
    only = SingleCellArgs(output=str(tmp_path / "only" / "out"), max_em_iter=MAX_ITER, collated=collated, gene_of=gene_of, gene_names=genes,
                          gene_counts=True)
    res = quantify_single_cell_from_record_batches(f, names, tl, [b[:4] for b in batches], only)
    assert same_counts(res[4]["gene_counts"], gene_walk(res[0], res[1], res[2], gene_of))
    meta = json.load(open(only.output + ".meta_info.json"))
    assert meta["gene_counts"] is True and meta["n_genes"] == n_genes and "umi_gene_keys" not in meta and "umi_dedup" not in meta
