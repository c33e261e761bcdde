"""The sessions' device arena (oarfish_amd/csrc/oem_dev_blob.h) under first capacities of 1: the testing library's
OEM_ARENA_RECORDS0 and OEM_ARENA_BYTES0 replace every instance's floor, so every part of every arena -- and the any-order
session's label blob -- grows on almost every append, and each growth copies a used prefix whose size is no multiple of
16.  The five sessions run on the hand-built inputs of their own "every cutting" tests, in three cuttings each, and must
give the one call's outputs exactly as those tests compare them."""
import numpy as np
import pytest

from oarfish_amd import _lib, synth
from tests import test_cells_barcodes_any_order_stream_gpu as any_order
from tests import test_cells_barcodes_stream_gpu as collated
from tests import test_cells_umis_stream_gpu as umis
from tests import test_records_stream_sort_gpu as sort
from tests.records_stream_sort_common import sort_records16
from tests.test_cells_records_names_gpu import pack

pytestmark = pytest.mark.gpu

TL40 = np.full(collated.EDGE_T, 2000, dtype=np.uint64)
F = collated.EDGE_FILTERS


@pytest.fixture
def floors_of_one(monkeypatch):
    monkeypatch.setenv("OEM_ARENA_RECORDS0", "1")
    monkeypatch.setenv("OEM_ARENA_BYTES0", "1")
    monkeypatch.setenv("OEM_KEEP_UNPACKED", "1")                        # (oem_debug_layout_hash reads the builders' streams)
    with _lib.testing():
        yield


def three_cuttings(n, two):
    """one record per batch, one batch, and two cuts that split a read and a cell"""
    assert len(two) == 2 and 0 < two[0] < two[1] < n
    return [list(range(1, n)), [], list(two)]


def survivors(rec):
    return np.flatnonzero((rec["flags"] & collated.U) == 0)


# ---- the five sessions: (got, want) compared as the session's own tests compare them, then the arena's lower bound -----
def run_sort(rec, names, sec, cuts, want, w_store):
    got = sort.session(want["F"], want["tl"], synth.cut_named_records(rec, names, cuts, secondary=sec))
    with got[0] as store:
        sort.same_outputs(got, want["one"])
        sort.same_small_store(store, w_store)
    S = survivors(rec)
    name_bytes = sum(int(names[1][i + 1] - names[1][i]) for i in S)
    assert got[4]["arena_bytes"] >= len(S) * (40 + 8 + 8 + 1) + name_bytes, cuts
    assert got[4]["arena_bytes"] < 1024 * (40 + 8 + 8 + 1), cuts        # the floors are in force: the default first capacity alone holds more


def run_cells(kind, st, edges, want):
    if kind == "collated":
        got = collated._session(collated._cut(st, edges), F, TL40, max_iter=20)
        collated._same(got, want, f"{kind}, edges {edges}")
    elif kind == "any_order":
        batches = collated._cut(st, edges)
        got = any_order._session(batches, F, TL40, max_iter=20)
        collated._same(got, want, f"{kind}, edges {edges}")
        any_order._check_info(got, batches, len(want["barcodes"]))      # arena_bytes >= survivors * (40 + 8 + 8 + 1 + 4)
    else:
        is_collated = kind == "collated_umis"
        got = umis._session(umis._cut(st, edges), F, TL40, is_collated, max_iter=20)
        umis._same_umis(got, want, f"{kind}, edges {edges}")
        if not is_collated:                                              # (a collated session reports no arena)
            S = want["S"]
            assert got["info"]["arena_bytes"] >= len(S) * (40 + 8 + 8 + 1 + 4 + 8) + sum(len(st["um"][i]) for i in S)
    if kind.startswith("any_order"):   # the floors are in force: the default first capacity of 4 Ki records alone holds more
        assert got["info"]["arena_bytes"] < 4096 * (40 + 8 + 8 + 1 + 4)


def cells_want(kind, st):
    if kind == "collated":
        return collated._expected(st, F, TL40, max_iter=20)
    if kind == "any_order":
        return any_order._expected(st, F, TL40, max_iter=20)
    return umis._expected(kind == "collated_umis", st, F, TL40, max_iter=20)


def test_the_sorting_names_session_in_three_cuttings(floors_of_one):
    rec, names, sec = sort_records16()
    one = sort.one_call(sort.FILTERS, sort.TL, rec, names, sec)
    with one[0] as w_store:
        for cuts in three_cuttings(16, (5, 11)):                         # the input is permuted: every cut splits reads
            run_sort(rec, names, sec, cuts, dict(one=one, F=sort.FILTERS, tl=sort.TL), w_store)


# the two cuts: inside read r2 of cell AAAA and inside read y of cell ACGT-1 (the collated input); the any-order input's
# reads and cells are scattered, so any two do; inside read r4 of cell A and inside read q of cell ACGT-1 (with UMIs)
@pytest.mark.parametrize("kind, two", [("collated", (2, 11)), ("any_order", (6, 11)), ("collated_umis", (4, 12)), ("any_order_umis", (4, 12))])
def test_the_cells_sessions_in_three_cuttings(floors_of_one, kind, two):
    st = {"collated": collated._stream16, "any_order": any_order._stream16}.get(kind, umis._stream17)()
    n = len(st["rec"])
    assert 16 <= n <= 20
    want = cells_want(kind, st)
    for cuts in three_cuttings(n, two):
        run_cells(kind, st, [0, *cuts, n], want)


def lead_unmapped(st):
    """st behind one unmapped record whose bytes no survivor may carry"""
    head = np.zeros(1, dtype=st["rec"].dtype)
    head["flags"] = collated.U
    return umis._ustream(np.concatenate([head, st["rec"]]), [collated.GARBAGE] + st["bc"], [collated.GARBAGE] + st["nm"],
                         np.concatenate([np.ones(1, dtype=np.uint8), st["sec"]]), [collated.GARBAGE] + st["um"])


@pytest.mark.parametrize("kind", ["sort", "collated", "any_order", "collated_umis", "any_order_umis"])
def test_unmapped_records_first_last_and_between_reads_one_record_per_batch(floors_of_one, kind):
    st = lead_unmapped(umis._stream17())
    n = len(st["rec"])
    unm = [i for i in range(n) if st["rec"]["flags"][i] & collated.U]
    assert unm == [0, 6, n - 1] and st["bc"][5] == st["bc"][7] and st["nm"][5] != st["nm"][7]   # first, between two reads of a cell, last
    if kind == "sort":
        names = pack(st["nm"])
        one = sort.one_call(F, TL40, st["rec"], names, st["sec"])
        with one[0] as w_store:
            run_sort(st["rec"], names, st["sec"], list(range(1, n)), dict(one=one, F=F, tl=TL40), w_store)
    else:
        run_cells(kind, st, list(range(n + 1)), cells_want(kind, st))
