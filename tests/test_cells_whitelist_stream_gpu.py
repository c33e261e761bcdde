"""GPU tests of the barcode rule in the any-order barcoded session (oem_cells_stream_set_whitelist / _whitelist_copy;
oarfish_amd/csrc/oem_barcode_correct.h, "The rule in a session"): raw barcodes corrected against a whitelist batch by batch.

finish() / cells() are held to the whitelist one call (oem_em_run_cells_records_whitelist_sparse, through
tests/test_correct_barcodes_gpu.py's _one_call) on the MAPPED records' arrays, with the session comparison of
tests/test_cells_barcodes_stream_gpu.py (_same) plus cell_dups, cell_corrected, cell_wl_id, cell_bc_corrected, the five
counts and the two info words.  The expected side never comes from a session."""
import ctypes as C
import itertools
import json
import threading

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth
from oarfish_amd.builder import ALN_RECORD
from oarfish_amd.em import BarcodeRuleC
from oarfish_amd.single_cell import SingleCellArgs, quantify_single_cell_from_record_batches
from tests.test_cells_barcodes_stream_gpu import EDGE_FILTERS, GARBAGE, SIZES, U, _cycled, _same, _stream
from tests.test_cells_records_gpu import COVS
from tests.test_cells_records_names_gpu import pack
from tests.test_collate_gpu import MAX_ITER, T
from tests.test_correct_barcodes import AMBIGUOUS, CORRECTED, EXACT, MISSING, NO_ID, NO_NEIGHBOUR, make_rule
from tests.test_correct_barcodes_gpu import _labels, _one_call
from tests.test_correct_barcodes_stream import A0, A1, A2, AB, BC, C0, C1, CD, STREAM, WL5

pytestmark = pytest.mark.gpu

T8 = 8
TL8 = np.full(T8, 2000, dtype=np.uint64)
GENE_OF8 = [0, 0, 1, 1, 2, 2, 3, 3]
REJECTED = (NO_NEIGHBOUR, AMBIGUOUS, MISSING)


# ---- the expected side, the session, the comparison ----------------------------------------------------------------------
def _wstream(rec, bc, nm, sec, um):
    st = _stream(rec, bc, nm, sec)
    st["um"] = list(um)
    return st


def _cut(st, edges, umis):
    cols = ("rec", "bc", "nm", "sec", "um") if umis else ("rec", "bc", "nm", "sec")
    return [tuple(st[k][a:b] for k in cols) for a, b in zip(edges[:-1], edges[1:])]


def _expected(st, wl, multi, filters, tl, umis=True, gene_of=None, correct=False, model=-1, mode="sort", max_iter=MAX_ITER):
    """the whitelist one call on the mapped records"""
    S = np.flatnonzero((st["rec"]["flags"] & U) == 0)
    n_unmapped = len(st["rec"]) - len(S)
    if not len(S):
        return dict(empty=True, n_unmapped=n_unmapped, counts=np.zeros(5, dtype=np.uint64), rejected=0, S=S)
    want = _one_call(wl, multi, filters, tl, st["rec"][S], pack([st["nm"][i] for i in S]), st["sec"][S], pack([st["bc"][i] for i in S]),
                     pack([st["um"][i] for i in S]) if umis else None, gene_of, correct, model=model, mode=mode, max_iter=max_iter)
    order, cro = want["order"].astype(np.int64), want["cell_rec_off"].astype(np.int64)
    wl_id, status = want["wl_id"], want["status"]
    cell_wl_id = wl_id[order[cro[:-1]]].astype(np.uint32)
    cell_of = {int(w): c for c, w in enumerate(cell_wl_id)}
    bc_corrected = np.zeros(len(cell_wl_id), dtype=np.uint64)       # over ALL accepted records of the cell, duplicates included
    for i in np.flatnonzero(status == CORRECTED):
        bc_corrected[cell_of[int(wl_id[i])]] += 1
    want.update(order64=S.astype(np.uint64)[order], barcodes=[wl[int(w)] for w in cell_wl_id], n_unmapped=n_unmapped, S=S, empty=False,
                cell_wl_id=cell_wl_id, cell_bc_corrected=bc_corrected, rejected=int(sum(want["counts"][k] for k in REJECTED)),
                dup_records=int((wl_id != NO_ID).sum()) - len(order), cell_dups=np.asarray(want["cell_dups"], dtype=np.uint64),
                cell_corrected=np.asarray(want["cell_corrected"], dtype=np.uint64))
    return want


def _session(batches, wl, multi, filters, tl, umis=True, gene_of=None, correct=False, model=-1, mode="sort", max_iter=MAX_ITER, push=None, **opts):
    rule = dict(gene_of=gene_of, umi_correct=correct) if umis else {}
    with oarfish_amd.CellsStream(len(tl), max_iter=max_iter, conv_thresh=1e-3, coverage=COVS[model], filters=filters, txp_len=tl, barcodes=True,
                                 collated=False, mode=mode, umis=umis, whitelist=wl, barcode_multi=bool(multi), **rule, **opts) as cs:
        if push is not None:
            push(cs)
        else:
            assert [cs.push_batch(*b) for b in batches] == list(range(len(batches)))
        cells = cs.finish()
        out = cs.cells()
        out.update(cells=cells, tables=cs.discard_tables(), info=cs.info())
    return out


def _same_whitelist(got, want, label, umis=True, correct=False, deferred=None):
    info = got["info"]
    assert np.array_equal(got["counts"], want["counts"]) and got["counts"].dtype == np.uint64, f"{label}: counts {got['counts']} {want['counts']}"
    assert info["barcode_rejected"] == want["rejected"], f"{label}: barcode_rejected"
    if deferred is not None:
        assert info["barcode_deferred"] == deferred, f"{label}: barcode_deferred"
    assert got["n_unmapped"] == want["n_unmapped"], f"{label}: n_unmapped"
    if want["empty"] or not len(want["barcodes"]):
        assert got["barcodes"] == [] and len(got["order"]) == 0 and list(got["cell_rec_off"]) == [0] and len(got["cell_wl_id"]) == 0, label
        assert len(got["cells"][0]) == 1 and len(got["cells"][1]) == 0, label
        return
    _same(got, want, label)
    for k in ("cell_wl_id", "cell_bc_corrected"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), f"{label}: {k}"
    if umis:
        assert np.array_equal(got["cell_dups"], want["cell_dups"]), f"{label}: cell_dups"
        assert info["umi_dup_reads"] == int(want["cell_dups"].sum()) and info["umi_dup_records"] == want["dup_records"], f"{label}: info"
    if correct:
        assert np.array_equal(got["cell_corrected"], want["cell_corrected"]), f"{label}: cell_corrected"
    # records accepted by the session = n_unmapped + rejected + positions of order + umi_dup_records
    assert info["alignments"] == got["n_unmapped"] + info["barcode_rejected"] + len(got["order"]) + info["umi_dup_records"], f"{label}: records"


# ---- 1. the hand-built stream: tests/test_correct_barcodes_stream.py's barcodes with reads, UMIs and transcripts around them --
def _umi(i):
    return bytes(b"ACGT"[(i >> s) & 3] for s in (0, 2, 4)) * 2      # two of them differ in two positions at least


A2N = A2[:-1] + b"N"
#           barcode name     secondary unmapped UMI  transcript
EXTRA = [(C0, b"r09", 1, 0, _umi(9), 2),       # 19  a secondary of read r09, ten records on
         (C0, b"d1", 0, 0, _umi(9), 1),        # 20  a PCR duplicate of r09
         (A2N, b"d2", 0, 0, _umi(0), 0),       # 21  a duplicate of r00 through a corrected barcode
         (C0, b"e1", 0, 0, b"GGGGGG", 4),      # 22  GGGGGT is one mismatch from GGGGGG, two reads against one, in one gene
         (C0, b"e2", 0, 0, b"GGGGGG", 5),      # 23
         (C0, b"e3", 0, 0, b"GGGGGT", 4),      # 24
         (b"", GARBAGE, 0, 1, GARBAGE, 0),     # 25  unmapped, without a barcode
         (AB, b"d3", 0, 0, _umi(1), 1),        # 26  a duplicate of the deferred r01, deferred itself
         (CD, b"r04", 1, 0, _umi(4), 5)]       # 27  a secondary of the deferred r04
BAD_REJECTED = (7, 11)                         # rejected in their batch: an empty name, a 0 byte in the UMI, a ref_id >= n_txps
N28 = len(STREAM) + len(EXTRA)


def _stream28():
    rng = np.random.default_rng(28)
    rows = [(bc, b"r%02d" % i, 0, un, _umi(i), i % T8) for i, (bc, un) in enumerate(STREAM)] + EXTRA
    rows = [(bc, GARBAGE, 1, 1, GARBAGE, tx) if un else (bc, nm, sec, un, um, tx) for bc, nm, sec, un, um, tx in rows]
    rec = np.zeros(N28, dtype=ALN_RECORD)
    for i, row in enumerate(rows):
        rec[i] = (row[5], 10, 1500, 1400, 1000 - int(rng.integers(0, 30)), 1500, U if row[3] else _lib.REC_HAS_SCORE, 0)
    st = _wstream(rec, *[[row[k] for row in rows] for k in (0, 1, 2, 4)])
    for i in BAD_REJECTED:
        st["nm"][i], st["um"][i] = b"", b"A\x00C"
        st["rec"]["ref_id"][i] = T8 + 3
    return st


VARIANTS28 = {"no umis": dict(umis=False), "umis under a rule": dict(umis=True, gene_of=GENE_OF8, correct=True)}


def test_the_hand_built_stream_holds_what_it_is_built_for():
    """On the input and the expected side alone (the barcodes' own story: tests/test_correct_barcodes_stream.py)."""
    st = _stream28()
    assert 25 <= N28 <= 32 and len(WL5) == 5 and all(len(w) == 12 for w in WL5)
    S = [int(i) for i in np.flatnonzero((st["rec"]["flags"] & U) == 0)]
    at = {i: k for k, i in enumerate(S)}
    w1 = _expected(st, WL5, 1, EDGE_FILTERS, TL8, max_iter=20, **VARIANTS28["umis under a rule"])
    w0 = _expected(st, WL5, 0, EDGE_FILTERS, TL8, max_iter=20, **VARIANTS28["umis under a rule"])
    s1, s0, id1 = w1["status"], w0["status"], w1["wl_id"]
    # tied when they arrive (no exact record of either label before them), decided by later batches' exact records
    assert st["bc"][1] == AB and not any(st["bc"][i] in (A0, A1) for i in S if i < 1) and s1[at[1]] == CORRECTED and id1[at[1]] == 0
    # the lead changes hands: C1 leads behind record 6, C0 at the end
    assert st["bc"][4] == CD and st["bc"][6] == C1 and [i for i in S if st["bc"][i] == C0][0] > 6 and id1[at[4]] == 3
    # still tied at the end: deferred, then rejected
    assert st["bc"][14] == BC and s1[at[14]] == AMBIGUOUS
    # the unmapped exact record 2 would make A0 / A1 tie (2 : 2) and A1 beat A2: it must not be counted
    assert st["rec"]["flags"][2] & U and st["bc"][2] == A1
    assert sum(st["bc"][i] == A0 for i in S) == 2 and sum(st["bc"][i] == A1 for i in S) == 1 and sum(st["bc"][i] == A2 for i in S) == 1
    # labels whose first accepted record is a deferred one: the cells' numbers depend on it
    assert list(w1["cell_wl_id"]) == [2, 0, 3, 4, 1]
    assert [st["bc"][i] for i in S if id1[at[i]] == 0][0] == AB and [st["bc"][i] for i in S if id1[at[i]] == 3][0] == CD
    # an N, an empty barcode, a length no label has, a double error
    assert st["bc"][5] == A2N and s1[at[5]] == CORRECTED and s1[at[7]] == MISSING and len(st["bc"][8]) == 13 and s1[at[8]] == NO_NEIGHBOUR
    assert s1[at[11]] == NO_NEIGHBOUR and s1[at[16]] == NO_NEIGHBOUR
    # rejected records with what would be an error on an accepted one
    for i in BAD_REJECTED:
        assert st["nm"][i] == b"" and b"\x00" in st["um"][i] and st["rec"]["ref_id"][i] >= T8 and s1[at[i]] in REJECTED and s0[at[i]] in REJECTED
    assert [s0[at[i]] for i in (1, 4, 14, 15, 18, 26, 27)] == [AMBIGUOUS] * 7
    assert int(w1["cell_dups"].sum()) >= 3 and int(w1["cell_corrected"].sum()) >= 1 and int(w1["cell_bc_corrected"].sum()) >= 7
    assert list(w1["counts"]) == [int((s1 == k).sum()) for k in range(5)] and w1["counts"][AMBIGUOUS] == 1


@pytest.mark.parametrize("variant", sorted(VARIANTS28))
@pytest.mark.parametrize("multi", (0, 1))
def test_every_cutting_of_the_hand_built_stream_at_up_to_two_positions(multi, variant):
    st, v = _stream28(), VARIANTS28[variant]
    want = _expected(st, WL5, multi, EDGE_FILTERS, TL8, max_iter=20, **v)
    cuttings = [c for k in (0, 1, 2) for c in itertools.combinations(range(1, N28), k)]
    assert len(cuttings) == 1 + 27 + 351
    for cuts in cuttings:
        got = _session(_cut(st, [0, *cuts, N28], v["umis"]), WL5, multi, EDGE_FILTERS, TL8, max_iter=20, **v)
        _same_whitelist(got, want, f"multi {multi}, {variant}, cuts {cuts}", v["umis"], v.get("correct", False), deferred=7 if multi else 0)


# ---- 2. the stated difference, and the barcode's own error -------------------------------------------------------------------
def _fails(batches, at, words, wl=WL5, multi=1):
    """the error comes out of finish (or of a push behind the faulty batch), with these words, and sticks"""
    with oarfish_amd.CellsStream(T8, max_iter=20, filters=EDGE_FILTERS, txp_len=TL8, barcodes=True, collated=False, umis=True, whitelist=wl,
                                 barcode_multi=bool(multi)) as cs:
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
        with pytest.raises(oarfish_amd.OemError):
            cs.cells()


def test_a_deferred_record_that_finish_rejects_is_checked_in_its_batch():
    """The stated difference: record 14 is still tied at the end, so the one call never looks at its name; the session has
    retained it in its batch, and a 0 byte in its name is the session's sticky error, by ticket and session-global index."""
    st = _stream28()
    st["nm"][14] = b"r\x00"
    edges = [0, 6, 12, 20, N28]
    want = _expected(st, WL5, 1, EDGE_FILTERS, TL8, max_iter=20)                    # the one call: no error
    assert want["status"][list(want["S"]).index(14)] == AMBIGUOUS
    _fails(_cut(st, edges, True), 2, ["ticket 2", "record 14", "0 byte", "name"])
    got = _session(_cut(st, edges, True), WL5, 0, EDGE_FILTERS, TL8, max_iter=20)   # multi 0: ambiguous in its batch, never looked at
    _same_whitelist(got, _expected(st, WL5, 0, EDGE_FILTERS, TL8, max_iter=20), "multi 0", deferred=0)


@pytest.mark.parametrize("i", [9, 14, 27])
def test_a_0_byte_in_a_mapped_records_barcode_names_ticket_and_session_index(i):
    st = _stream28()
    st["bc"][i] = st["bc"][i][:3] + b"\x00" + st["bc"][i][4:]
    edges = [0, 6, 12, 20, N28]
    ticket = max(k for k, e in enumerate(edges[:-1]) if e <= i)
    _fails(_cut(st, edges, True), ticket, [f"ticket {ticket}", f"record {i}", "0 byte", "barcode"])
    st = _stream28()
    st["bc"][2] = b"AA\x00A"                                                           # unmapped: never examined
    got = _session(_cut(st, edges, True), WL5, 1, EDGE_FILTERS, TL8, max_iter=20)
    _same_whitelist(got, _expected(st, WL5, 1, EDGE_FILTERS, TL8, max_iter=20), "an unmapped record's barcode", deferred=7)


# ---- 3. launch and wavefront edges, one batch each ---------------------------------------------------------------------------
EDGE_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)
X0, X1, Y0 = b"ACGTACGTACGT", b"ACGTACGTACGA", b"TTGGCCAATTGG"      # X0 / X1 are one substitution apart
BETWEEN = b"ACGTACGTACGC"                                           # a neighbour of both
Y_ERR = [Y0[:p] + b"N" + Y0[p + 1:] for p in range(12)]             # Y0 their only neighbour


def _edge_stream(special, k, n_exact=70):
    """k special records -- the first and the last record of the batch among them -- between exact ones"""
    bcs = [X0] * n_exact + [Y0] * 3
    slots = sorted(set(np.linspace(0, len(bcs) + k - 1, k).astype(int).tolist())) if k else []
    assert len(slots) == k
    out, it, s = [], iter(bcs), set(slots)
    for pos in range(len(bcs) + k):
        out.append(special[pos % len(special)] if pos in s else next(it))
    if k:
        assert out[0] in special and (k == 1 or out[-1] in special)
    n = len(out)
    rng = np.random.default_rng(k)
    rec = np.zeros(n, dtype=ALN_RECORD)
    for i in range(n):
        rec[i] = (int(rng.integers(0, T8)), 10, 1500, 1400, 1000 - int(rng.integers(0, 30)), 1500, _lib.REC_HAS_SCORE, 0)
    return _wstream(rec, out, [b"q%04d" % i for i in range(n)], [0] * n, [_umi(i % 61) for i in range(n)])


@pytest.mark.parametrize("k", EDGE_COUNTS)
@pytest.mark.parametrize("kind", ["deferred", "misses"])
def test_deferred_and_miss_counts_around_the_wavefront_and_workgroup_edges(kind, k):
    wl = [X0, X1, Y0]
    st = _edge_stream([BETWEEN] if kind == "deferred" else Y_ERR, k)
    n = len(st["rec"])
    for multi in (1, 0) if kind == "deferred" else (1,):
        want = _expected(st, wl, multi, EDGE_FILTERS, TL8, max_iter=20)
        deferred = k if kind == "deferred" and multi else 0
        if kind == "deferred":
            assert want["counts"][CORRECTED if multi else AMBIGUOUS] == k
        else:
            assert want["counts"][CORRECTED] == k
        got = _session(_cut(st, [0, n], True), wl, multi, EDGE_FILTERS, TL8, max_iter=20)
        _same_whitelist(got, want, f"{kind} {k}, multi {multi}, one batch", deferred=deferred)
    if k in (1, 65, 257):       # the pending list over three batches: the deferred records' arena positions are not their batch's
        got = _session(_cut(st, [0, n // 3, n // 2, n], True), wl, 1, EDGE_FILTERS, TL8, max_iter=20)
        _same_whitelist(got, _expected(st, wl, 1, EDGE_FILTERS, TL8, max_iter=20), f"{kind} {k}, three batches")


def test_batches_and_sessions_where_nothing_is_retained():
    st = _stream28()
    n = N28
    # a batch all of whose mapped records are rejected (7 and 8: missing, a length no label has), with their garbage
    st["nm"][8], st["um"][8] = b"", b"\x00"
    edges = [0, 7, 9, 17, 18, n]                    # [17, 18) is a batch of one unmapped record
    got = _session(_cut(st, edges, True), WL5, 1, EDGE_FILTERS, TL8, max_iter=20)
    _same_whitelist(got, _expected(st, WL5, 1, EDGE_FILTERS, TL8, max_iter=20), "a rejected batch, an unmapped batch", deferred=7)
    # nothing is accepted: rejected in the batches, or deferred and rejected at finish
    keep = [i for i in range(n) if st["rec"]["flags"][i] & U or st["bc"][i] in (b"", BC, b"TTAAAAAAAAAA") or len(st["bc"][i]) == 13]
    sub = _wstream(st["rec"][keep], *[[st[k][i] for i in keep] for k in ("bc", "nm")], st["sec"][keep], [st["um"][i] for i in keep])
    wl = [A1, A2, C0]                                # BC ties 0 : 0
    want = _expected(sub, wl, 1, EDGE_FILTERS, TL8, max_iter=20)
    assert want["counts"][EXACT] == want["counts"][CORRECTED] == 0 and want["counts"][AMBIGUOUS] == 1 and want["rejected"] == len(want["S"])
    for edges in ([0, len(keep)], [0, 2, 3, len(keep)]):
        got = _session(_cut(sub, edges, True), wl, 1, EDGE_FILTERS, TL8, max_iter=20)
        _same_whitelist(got, want, f"nothing accepted, {edges}", deferred=1)
    # unmapped records only, and no records at all
    um = [i for i in range(n) if st["rec"]["flags"][i] & U]
    only = _wstream(st["rec"][um], *[[st[k][i] for i in um] for k in ("bc", "nm")], st["sec"][um], [st["um"][i] for i in um])
    got = _session(_cut(only, [0, 1, len(um)], True), WL5, 1, EDGE_FILTERS, TL8, max_iter=20)
    _same_whitelist(got, _expected(only, WL5, 1, EDGE_FILTERS, TL8), "unmapped only", deferred=0)
    assert got["n_unmapped"] == len(um) == 3 and got["info"]["barcode_rejected"] == 0
    got = _session([], WL5, 1, EDGE_FILTERS, TL8, max_iter=20)
    assert got["barcodes"] == [] and not got["counts"].any()


# ---- 4. synthetic input --------------------------------------------------------------------------------------------------------
N_CELLS, READS_PER_CELL = 4, 180


@pytest.fixture(scope="module")
def raw():
    """Four cells of about 180 reads and two whose barcodes are on no whitelist, interleaved; PCR duplicates and UMI errors;
    substitutions and Ns in the barcodes; for every cell's label a PLANTED label one substitution from it, with a few
    exact reads of its own, and reads whose barcode is a third byte at that position: between the two, deferred.  Every
    11th record is unmapped and carries garbage."""
    reads = [READS_PER_CELL + 7 * k for k in range(N_CELLS)] + [30, 20]
    stores = [synth.make_cells(1, r, T, kbar=4.0, seed=701 + k) for k, r in enumerate(reads)]
    co, rps, tids, ps, nnz = [0], [np.zeros(1, dtype=np.uint64)], [], [], 0
    for _, rp, tid, p in stores:
        rps.append(rp[1:] + np.uint64(nnz))
        tids.append(tid)
        ps.append(p)
        nnz += len(tid)
        co.append(co[-1] + len(rp) - 1)
    cr = synth.make_cell_records((np.array(co, dtype=np.uint64), np.concatenate(rps), np.concatenate(tids), np.concatenate(ps)), T, seed=17)
    rec, names, sec, cro = synth.shuffle_cell_records(cr, seed=4, style="illumina")
    whitelist = _labels(96, length=16, seed=33)
    cell_bc = whitelist[20:20 + N_CELLS] + [b"GGGGGGNNGGGGGGGG", whitelist[3][:15]]
    r1, n1, s1, bc1, _ = synth.interleave_cells(rec, names, sec, cro, cell_bc, seed=6, how="uniform")
    r2, n2, s2, bc2, umis, _ = synth.add_umi_duplicates(r1, n1, s1, bc1, rate=0.3, seed=19)
    umis = synth.add_umi_errors(umis, 0.2, seed=9, names=n2, barcodes=bc2)
    bc3 = synth.add_barcode_errors(bc2, 0.12, 0.04, seed=8, names=n2)
    n = len(r2)
    as_list = lambda p: [np.asarray(p[0]).tobytes()[int(p[1][i]):int(p[1][i + 1])] for i in range(n)]   # noqa: E731
    bcs, clean, nms, ums = as_list(bc3), as_list(bc2), as_list(n2), as_list(umis)
    swap = {ord("A"): b"C", ord("C"): b"G", ord("G"): b"T", ord("T"): b"A"}
    planted, between = {}, {}
    for c, lab in enumerate(cell_bc[:N_CELLS]):
        p = 3 + 2 * c
        planted[lab] = lab[:p] + swap[lab[p]] + lab[p + 1:]
        between[lab] = lab[:p] + swap[planted[lab][p]] + lab[p + 1:]
        assert planted[lab] not in whitelist and between[lab] not in whitelist
    whitelist = whitelist + [planted[lab] for lab in cell_bc[:N_CELLS]]
    for i in range(n):                                        # by read, so that a read's records stay together
        h = sum(nms[i]) * 2654435761 % 97
        if clean[i] in planted and h < 9:
            bcs[i] = between[clean[i]] if h < 7 else planted[clean[i]]
    r2 = r2.copy()
    for i in range(5, n, 11):
        r2["flags"][i] |= U
        bcs[i], nms[i], ums[i] = (whitelist[20] if i % 2 else GARBAGE), GARBAGE, GARBAGE
    st = _wstream(r2, bcs, nms, s2, ums)
    st["rec"].setflags(write=False)
    return dict(st=st, filters=cr.filters, tl=cr.txp_len, whitelist=whitelist, gene_of=synth.gene_of_txps(T), clean=clean, refs={})


def _ref(fx, multi=1, model=-1, mode="sort", umis=True, rule=True):
    key = (multi, model, mode, umis, rule)
    if key not in fx["refs"]:
        kw = dict(gene_of=fx["gene_of"], correct=True) if umis and rule else {}
        want = _expected(fx["st"], fx["whitelist"], multi, fx["filters"], fx["tl"], umis=umis, model=model, mode=mode, **kw)
        c = want["counts"]
        assert c[EXACT] > 1000 and c[CORRECTED] > 100 and c[NO_NEIGHBOUR] > 20 and len(want["barcodes"]) >= N_CELLS + 1
        assert 1500 < len(fx["st"]["rec"]) < 12000 and want["n_unmapped"] > 100
        if umis:
            assert int(want["cell_dups"].sum()) > 50
        fx["refs"][key] = want
    return fx["refs"][key]


def _n_between(fx):
    """the mapped records with two neighbours: what a multi session defers"""
    st, wl = fx["st"], set(fx["whitelist"])
    out = 0
    for i in np.flatnonzero((st["rec"]["flags"] & U) == 0):
        b = st["bc"][i]
        if b and b not in wl and len(b) == 16:
            out += sum(1 for lab in wl if sum(x != y for x, y in zip(lab, b)) == 1 and [y for x, y in zip(b, lab) if x != y][0] in b"ACGT") >= 2
    return out


def _kw(fx, rule=True):
    return dict(gene_of=fx["gene_of"], correct=True) if rule else {}


@pytest.mark.parametrize("mode", ["sort", "adjacent"])
@pytest.mark.parametrize("model", [-1, 1])
def test_synthetic_input_in_cycled_batch_sizes(raw, model, mode):
    fx = raw
    st = fx["st"]
    if mode == "adjacent" and "adj" not in fx:   # name-collated inside every cell of the accepted records: reads adjacent in the stream
        order = sorted(range(len(st["rec"])), key=lambda i: (fx["clean"][i], st["nm"][i], int(st["sec"][i])))
        adj = _wstream(st["rec"][order], *[[st[k][i] for i in order] for k in ("bc", "nm")], st["sec"][order], [st["um"][i] for i in order])
        fx["adj"] = dict(fx, st=adj, refs={})
    fx = fx["adj"] if mode == "adjacent" else fx
    st = fx["st"]
    want = _ref(fx, 1, model, mode)
    n_def = _n_between(fx)
    batches = _cut(st, _cycled(len(st["rec"])), True)
    assert {len(b[0]) for b in batches[:-1]} == set(SIZES)
    got = _session(batches, fx["whitelist"], 1, fx["filters"], fx["tl"], model=model, mode=mode, **_kw(fx))
    assert got["info"]["barcode_deferred"] == n_def > 20
    _same_whitelist(got, want, f"model {model}, {mode}", correct=True, deferred=n_def)


@pytest.mark.parametrize("multi,umis,rule", [(0, True, True), (1, False, False), (1, True, False)])
def test_synthetic_input_under_the_other_rules(raw, multi, umis, rule):
    fx, st = raw, raw["st"]
    want = _ref(fx, multi, umis=umis, rule=rule)
    got = _session(_cut(st, _cycled(len(st["rec"])), umis), fx["whitelist"], multi, fx["filters"], fx["tl"], umis=umis, **_kw(fx, rule))
    _same_whitelist(got, want, f"multi {multi}, umis {umis}, rule {rule}", umis, rule, deferred=_n_between(fx) if multi else 0)


def test_many_groups_and_a_growing_arena_and_pending_list(raw, monkeypatch):
    """group_cells = 1 and a small group_nnz: every cell is a group.  The testing library's floors of 8 records and 64 bytes
    make the arena and the pending list grow many times (tests/test_session_arena_growth_gpu.py's knobs)."""
    fx, st = raw, raw["st"]
    want = _ref(fx)
    n_def = _n_between(fx)
    monkeypatch.setenv("OEM_ARENA_RECORDS0", "8")
    monkeypatch.setenv("OEM_ARENA_BYTES0", "64")
    with _lib.testing():
        got = _session(_cut(st, list(range(0, len(st["rec"]), 97)) + [len(st["rec"])], True), fx["whitelist"], 1, fx["filters"], fx["tl"],
                       group_cells=1, group_nnz=500, **_kw(fx))
    _same_whitelist(got, want, "many groups, growth", correct=True, deferred=n_def)
    assert got["info"]["groups"] == len(want["barcodes"]) > 3
    n_ret = len(want["S"]) - int(want["counts"][NO_NEIGHBOUR] + want["counts"][MISSING])
    assert got["info"]["arena_bytes"] > 52 * n_ret           # a record, its index, its id: the arena held the retained records


def test_four_threads_push_and_the_tickets_give_the_order(raw):
    fx, st = raw, raw["st"]
    n = len(st["rec"])
    batches = _cut(st, list(range(0, n, 300)) + [n], True)
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

    got = _session(None, fx["whitelist"], 1, fx["filters"], fx["tl"], push=push, **_kw(fx))
    assert sorted(tickets) == list(range(len(batches)))
    by_ticket = [batches[k] for k in np.argsort(tickets)]
    pushed = _wstream(np.concatenate([b[0] for b in by_ticket]), *[sum((list(b[k]) for b in by_ticket), []) for k in (1, 2)],
                      np.concatenate([b[3] for b in by_ticket]), sum((list(b[4]) for b in by_ticket), []))
    _same_whitelist(got, _expected(pushed, fx["whitelist"], 1, fx["filters"], fx["tl"], **_kw(fx)), "four threads", correct=True)


# ---- 5. a whitelist that holds exactly the clean barcodes --------------------------------------------------------------------
def test_exact_only_input_gives_the_plain_any_order_sessions_cells(raw):
    fx, st0 = raw, raw["st"]
    st = _wstream(st0["rec"], [b if (b and b"\x00" not in b) else b"GG" for b in fx["clean"]], st0["nm"], st0["sec"], st0["um"])
    for i in np.flatnonzero((st["rec"]["flags"] & U) != 0):
        st["bc"][i] = GARBAGE
    mapped = [st["bc"][i] for i in np.flatnonzero((st["rec"]["flags"] & U) == 0)]
    wl = sorted(set(mapped))                                   # the whitelist's order is not the cells'
    batches = _cut(st, _cycled(len(st["rec"])), True)
    with oarfish_amd.CellsStream(T, max_iter=MAX_ITER, filters=fx["filters"], txp_len=fx["tl"], barcodes=True, collated=False, umis=True) as cs:
        for b in batches:
            cs.push_batch(*b)
        cells = cs.finish()
        plain = cs.cells()
    got = _session(batches, wl, 1, fx["filters"], fx["tl"])
    assert got["barcodes"] == plain["barcodes"] == list(dict.fromkeys(mapped))
    for k in ("order", "cell_rec_off", "group_off", "cell_group_off", "kept", "cell_dups"):
        assert np.array_equal(got[k], plain[k]), k
    assert np.array_equal(got["cells"][0], cells[0]) and np.array_equal(got["cells"][1], cells[1])
    assert list(got["counts"]) == [len(mapped), 0, 0, 0, 0] and not got["cell_bc_corrected"].any()
    assert got["info"]["barcode_rejected"] == got["info"]["barcode_deferred"] == 0


# ---- 6. state and argument errors ----------------------------------------------------------------------------------------------
def _rule(wl, multi=0, alphabet=None):
    return make_rule(dict(whitelist=wl, alphabet=alphabet), multi)


def test_state_and_argument_errors():
    L = _lib.lib()
    st = _stream28()
    batch = _cut(st, [0, 6], False)[0]
    ok, keep = _rule(WL5, 1)
    err = lambda: L.oem_last_error().decode()   # noqa: E731
    out_id, out_corr, out_counts = np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.uint64), np.zeros(5, dtype=np.uint64)
    copy = lambda cs: L.oem_cells_stream_whitelist_copy(cs._h, out_id.ctypes.data, out_corr.ctypes.data, out_counts.ctypes.data)   # noqa: E731
    # a plain session, a records session, the collated barcoded session: OEM_ERR_STATE
    with oarfish_amd.CellsStream(T8) as cs:
        assert L.oem_cells_stream_set_whitelist(cs._h, C.addressof(ok)) == _lib.OEM_ERR_STATE
        assert copy(cs) == _lib.OEM_ERR_STATE
    with oarfish_amd.CellsStream(T8, filters=EDGE_FILTERS, txp_len=TL8) as cs:
        assert L.oem_cells_stream_set_whitelist(cs._h, C.addressof(ok)) == _lib.OEM_ERR_STATE and "any-order" in err()
    with oarfish_amd.CellsStream(T8, filters=EDGE_FILTERS, txp_len=TL8, barcodes=True) as cs:
        assert L.oem_cells_stream_set_whitelist(cs._h, C.addressof(ok)) == _lib.OEM_ERR_STATE
        assert "collated" in err() and "oem_cells_stream_set_barcodes_any_order" in err()
        assert copy(cs) == _lib.OEM_ERR_STATE
    # the rule's own checks and the whitelist errors found on the device: OEM_ERR_ARG, and the session stays usable
    with oarfish_amd.CellsStream(T8, max_iter=20, filters=EDGE_FILTERS, txp_len=TL8, barcodes=True, collated=False) as cs:
        assert L.oem_cells_stream_set_whitelist(cs._h, None) == _lib.OEM_ERR_ARG and "NULL" in err()
        for bad, words in ((_rule([]), "holds a label"), (_rule([b"ACGT", b""]), "label 1 of the whitelist is empty"),
                           (_rule([b"A" * 65]), "more than 64 bytes"), (_rule(WL5, 2), "neither 0 nor 1"),
                           (_rule(WL5, 0, b"ACGA"), "repeats"), (_rule([b"ACGT", b"AC\x00T"]), "label 1 of the whitelist contains a 0 byte"),
                           (_rule([b"ACGT", b"TTTT", b"ACGT"]), "labels 0 and 2 of the whitelist are equal")):
            assert L.oem_cells_stream_set_whitelist(cs._h, C.addressof(bad[0])) == _lib.OEM_ERR_ARG and words in err(), (words, err())
            assert "oem_cells_stream_set_whitelist" in err()
        assert copy(cs) == _lib.OEM_ERR_STATE                                           # no whitelist yet
        assert L.oem_cells_stream_set_whitelist(cs._h, C.addressof(ok)) == _lib.OEM_OK, err()
        assert L.oem_cells_stream_set_whitelist(cs._h, C.addressof(ok)) == _lib.OEM_ERR_STATE and "already" in err()   # a second time
        assert copy(cs) == _lib.OEM_ERR_STATE and "finish" in err()                   # before finish
        cs._whitelist = True
        cs.push_batch(*batch)
        cs.finish()
        assert copy(cs) == _lib.OEM_OK and L.oem_cells_stream_whitelist_copy(cs._h, None, None, None) == _lib.OEM_OK   # each output may be NULL
        assert list(out_counts) == list(cs.cells()["counts"]) and out_counts.sum() == 5
        assert L.oem_cells_stream_set_whitelist(cs._h, C.addressof(ok)) == _lib.OEM_ERR_STATE and "finished" in err()  # after finish
    # after a push; in either order with set_umis / set_umi_rule (the constructor sets the whitelist last: here it comes first)
    with oarfish_amd.CellsStream(T8, max_iter=20, filters=EDGE_FILTERS, txp_len=TL8, barcodes=True, collated=False) as cs:
        cs.push_batch(*batch)
        assert L.oem_cells_stream_set_whitelist(cs._h, C.addressof(ok)) == _lib.OEM_ERR_STATE and "pushed" in err()
    with oarfish_amd.CellsStream(T8, max_iter=20, filters=EDGE_FILTERS, txp_len=TL8, barcodes=True, collated=False) as cs:
        assert L.oem_cells_stream_set_whitelist(cs._h, C.addressof(ok)) == _lib.OEM_OK
        assert L.oem_cells_stream_set_umis(cs._h) == _lib.OEM_OK
        cs._whitelist = cs._umis = True
        for b in _cut(st, [0, 9, N28], True):
            cs.push_batch(*b)
        cells = cs.finish()
        got = cs.cells()
        got.update(cells=cells, tables=cs.discard_tables(), info=cs.info())
    _same_whitelist(got, _expected(st, WL5, 1, EDGE_FILTERS, TL8, max_iter=20), "the whitelist before the UMIs", deferred=7)
    # the rule's arrays are copied: the caller's are gone before the first push
    with oarfish_amd.CellsStream(T8, max_iter=20, filters=EDGE_FILTERS, txp_len=TL8, barcodes=True, collated=False, umis=True, whitelist=list(WL5),
                                 barcode_multi=True) as cs:
        import gc
        gc.collect()
        scratch = [np.full(4096, 0x5A, dtype=np.uint8) for _ in range(8)]   # noqa: F841
        for b in _cut(st, [0, 9, N28], True):
            cs.push_batch(*b)
        cs.finish()
        assert cs.cells()["barcodes"] == [WL5[w] for w in (2, 0, 3, 4, 1)]
    del keep
    # the Python layer's own refusals
    for kw, words in ((dict(whitelist=WL5), "barcodes=True"), (dict(whitelist=WL5, barcodes=True), "collated=False"),
                      (dict(barcodes=True, collated=False, barcode_multi=True), "barcode_multi goes with whitelist")):
        with pytest.raises(ValueError, match=words):
            oarfish_amd.CellsStream(T8, filters=EDGE_FILTERS, txp_len=TL8, **kw)


# ---- 7. the driver ----------------------------------------------------------------------------------------------------------------
def test_the_driver_writes_the_whitelists_labels_and_the_counts(raw, tmp_path):
    fx, st = raw, raw["st"]
    want = _ref(fx)
    names = [f"t{i}" for i in range(T)]
    batches = _cut(st, _cycled(len(st["rec"])), True)
    args = SingleCellArgs(output=str(tmp_path / "out"), max_em_iter=MAX_ITER, collated=False, umis=True, gene_of=fx["gene_of"], umi_correct=True,
                          whitelist=fx["whitelist"], barcode_multi=True)
    got = quantify_single_cell_from_record_batches(fx["filters"], names, fx["tl"], batches, args)
    assert got[4]["barcodes"] == want["barcodes"] and np.array_equal(got[4]["cell_wl_id"], want["cell_wl_id"])
    assert np.array_equal(got[0], want["cells"][0]) and np.array_equal(got[1], want["cells"][1])
    rows = open(args.output + ".barcodes.txt").read().split("\n")[:-1]
    assert rows == [b.decode() for b in want["barcodes"]] and all(r.encode() in fx["whitelist"] for r in rows)
    raw_only = {b for b in st["bc"] if b and b not in fx["whitelist"] and b"\x00" not in b}
    assert raw_only and not any(r.encode() in raw_only for r in rows)        # never a record's raw bytes
    meta = json.load(open(args.output + ".meta_info.json"))
    assert meta["barcode_whitelist_labels"] == len(fx["whitelist"]) and meta["barcode_multi"] is True
    for k, word in enumerate(("exact", "corrected", "no_neighbour", "ambiguous", "missing")):
        assert meta["barcode_" + word] == int(want["counts"][k])
    assert meta["umi_duplicate_reads"] == int(want["cell_dups"].sum())
    with pytest.raises(ValueError, match="collated=False"):
        SingleCellArgs(output="x", whitelist=fx["whitelist"])
