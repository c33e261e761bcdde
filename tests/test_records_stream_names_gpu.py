"""GPU tests of the names session (oem_records_stream_set_names / _push_names / _finish_names / _names_copy,
``RecordsStream(names=True)``, ``bulk.quantify_bulk_alignments_from_record_batches``): however the records and names are
cut into batches -- inside a read too -- finish gives what oem_store_create_records_names gives under ADJACENT on the
batches concatenated in ticket order: group_off, kept, the discard table, every parse field, the row names, the joined
CSR bit for bit and the store."""
import ctypes as C
import re
import threading

import numpy as np
import pytest

from oarfish_amd import _lib, synth, writers
from oarfish_amd.builder import ALN_RECORD, RecordsStream, StoreBuilder
from oarfish_amd.types import DeviceStore

from tests.common import assert_counts_close
from tests.records_stream_names_common import HEADS16, INPUT16, SIZES16, T, U, cuttings16, records16
from tests.test_filter_groups_gpu import _compare
from tests.test_records_stream_gpu import JOIN_TIMEOUT, _hash, finish_csr

pytestmark = pytest.mark.gpu

FILTERS = dict(five_prime_clip=2 ** 32 - 1, three_prime_clip=2 ** 62, score_threshold=0.95, min_aligned_fraction=0.5,
               min_aligned_len=50, which_strand=0, score_prob_denom=5.0)
TL = np.full(T, 2000, dtype=np.uint64)
PARSE_FIELDS = ("n_unmapped", "n_parsed", "n_groups", "n_reads", "unique_alignments", "n_checked")


def names_list(names):
    blob, off = names
    return [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def pack(names):
    off = np.zeros(len(names) + 1, dtype=np.uint64)
    np.cumsum([len(nm) for nm in names], out=off[1:])
    return np.frombuffer(b"".join(names), dtype=np.uint8), off


def concat(batches):
    rec = np.concatenate([b[0] for b in batches]) if batches else np.zeros(0, dtype=ALN_RECORD)
    nl = [nm for b in batches for nm in names_list(b[1])]
    return rec, pack(nl)


def simple_records(n, unmapped=None):
    rec = np.zeros(n, dtype=ALN_RECORD)
    i = np.arange(n)
    rec["ref_id"], rec["aln_start"], rec["aln_end"], rec["aln_span"] = i % T, 10, 1500, 1400
    rec["score"], rec["seq_len"], rec["flags"] = 1000 - (i % 3), 1500, _lib.REC_HAS_SCORE
    if unmapped is not None:
        rec["flags"][np.asarray(unmapped, dtype=bool)] = U
        rec["ref_id"][np.asarray(unmapped, dtype=bool)] = 0xFFFFFFFF
    return rec


def session(F, tl, batches, check=100_000, coverage=None, finish=None, **kw):
    """(store, kept, dt, parse, info) of a names session over the batches"""
    with RecordsStream(F, tl, coverage=coverage, names=True, sort_check_num=check, **kw) as s:
        tickets = [s.push(r, names=nm) for r, nm in batches]
        assert tickets == list(range(len(batches)))
        store, kept, dt, parse = s.finish(**(finish or {}))
        return store, kept, dt, parse, s.info()


def same_outputs(got, want):
    """group_off, kept, the discard table, every parse field and the row names"""
    (_, kept, dt, parse), (_, w_kept, w_dt, w_parse) = got[:4], want[:4]
    assert parse.order is None
    assert np.array_equal(parse.group_off, w_parse.group_off) and parse.group_off.dtype == np.uint64
    assert np.array_equal(kept, w_kept) and dt == w_dt
    for f in PARSE_FIELDS:
        assert getattr(parse, f) == getattr(w_parse, f), f
    assert np.array_equal(parse.read_names[1], w_parse.read_names[1]) and np.array_equal(parse.read_names[0], w_parse.read_names[0])


# ---- 1: exhaustive cuts ---------------------------------------------------------------------------------------------
def test_every_cutting_of_the_16_record_input_gives_the_one_calls_outputs():
    rec, names = records16()
    want = DeviceStore.from_named_records(FILTERS, TL, rec, names, mode="adjacent")
    w_store, w_kept, w_dt, w_parse = want
    # the rule in NumPy: runs of equal names among the mapped records
    nl = np.array([nm for _, nm in INPUT16], dtype=object)
    mapped = np.flatnonzero((rec["flags"] & U) == 0)
    head = np.concatenate([[True], nl[mapped][1:] != nl[mapped][:-1]])
    rule_off = np.concatenate([np.flatnonzero(head), [len(mapped)]]).astype(np.uint64)
    assert np.array_equal(rule_off, w_parse.group_off) and list(np.diff(rule_off)) == SIZES16
    assert [int(mapped[int(p)]) for p in rule_off[:-1]] == HEADS16
    rule_rows = [nl[mapped[int(rule_off[g])]] for g in np.flatnonzero(w_kept)]
    assert names_list(w_parse.read_names) == rule_rows and len(rule_rows) == 5 and w_parse.n_unmapped == 5
    dims = (w_store.n_reads, w_store.nnz, w_store.n_txps)
    w_store.close()
    assert dims == (5, int(w_kept.sum()), T)
    for cuts in cuttings16():
        batches = synth.cut_named_records(rec, names, cuts)
        got = session(FILTERS, TL, batches)
        with got[0] as store:
            same_outputs(got, want)
            assert np.array_equal(got[3].group_off, rule_off) and names_list(got[3].read_names) == rule_rows, cuts
            assert (store.n_reads, store.nnz, store.n_txps) == dims, cuts
            assert got[4]["batches"] == len(cuts) + 1 and got[4]["records"] == 16 and got[4]["groups"] == 5
            assert got[4]["row_name_bytes"] == len(got[3].read_names[0])


# ---- the fixture of 2, 3, 6 and 8 -----------------------------------------------------------------------------------
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 3001]


def cut_sizes(rec, names, sizes):
    """cut at record positions into batches of these sizes (the last entry repeats until the end)"""
    cuts, at, k = [], 0, 0
    while at < len(rec):
        at = min(at + sizes[min(k, len(sizes) - 1)], len(rec))
        k += 1
        if at < len(rec):
            cuts.append(at)
    return synth.cut_named_records(rec, names, cuts)


@pytest.fixture(scope="module")
def fx():
    sr = synth.make_records(synth.make_store(20_000, 500, seed=411), seed=412)
    rec, names, _ = synth.make_named_records(sr, seed=413, unmapped_rate=0.05)
    batches = cut_sizes(rec, names, SIZES)
    planted = simple_records(3, [1, 1, 1])
    batches.insert(12, (planted, pack([b"", b"x", b""])))                # a batch of three unmapped records
    rec, names = concat(batches)
    one = {}

    def one_call(coverage=None, check=100_000, **kw):
        key = (coverage, check, tuple(sorted(kw.items())))
        if key not in one:
            store, kept, dt, parse = DeviceStore.from_named_records(sr.filters, sr.txp_len, rec, names, mode="adjacent",
                                                                    sort_check_num=check, coverage=coverage, **kw)
            one[key] = (store, kept, dt, parse)
        return one[key]
    yield dict(sr=sr, rec=rec, names=names, batches=batches, one_call=one_call, T=len(sr.txp_len))
    for store, *_ in one.values():
        store.close()


def test_the_fixture_cuts_reads_and_unmapped_records_and_misaligns_the_pieces(fx):
    rec, batches = fx["rec"], fx["batches"]
    sizes = [len(b[0]) for b in batches]
    assert sizes[:10] == SIZES[:10] and sizes[12] == 3 and sizes.count(3001) >= 10
    nl = names_list(fx["names"])
    mapped = (rec["flags"] & U) == 0
    cuts = np.cumsum(sizes)[:-1]
    idx = np.flatnonzero(mapped)
    inside = 0
    for p in cuts:
        k = np.searchsorted(idx, p)                                      # the first mapped record at or after the cut
        inside += bool(0 < k < len(idx) and nl[idx[k - 1]] == nl[idx[k]])
    assert inside >= 5
    assert sum(1 for p in cuts if p < len(rec) and not mapped[p]) >= 1    # a cut directly before an unmapped record
    assert sum(1 for p in cuts if p > 0 and not mapped[p - 1]) >= 1       # ... and directly after one
    # the pieces: a group is closed by the batch that holds the next group's head, the last group by finish
    _, kept, _, parse = fx["one_call"]()
    heads = idx[parse.group_off[:-1].astype(np.int64)]
    edges = np.concatenate([[0], np.cumsum(sizes)])
    piece = np.append(np.searchsorted(edges, heads[1:], side="right") - 1, len(batches))
    aln_base = np.concatenate([[0], np.cumsum(kept.astype(np.int64))])[:-1]
    name_len = np.array([len(nl[h]) for h in heads]) * (kept > 0)
    byte_base = np.concatenate([[0], np.cumsum(name_len)])[:-1]
    first = np.flatnonzero(np.concatenate([[True], piece[1:] != piece[:-1]]))       # each piece's first group
    assert len(first) >= 15 and set(aln_base[first] % 4) == {0, 1, 2, 3}
    assert (byte_base[first] % 16 != 0).any()      # (36-byte names: the bases are multiples of 4; test 1's names are of odd lengths)


# ---- 2: the join, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("coverage", [None, "logistic"])
def test_the_joined_csr_is_the_host_builders_on_the_one_calls_groups(fx, coverage):
    sr = fx["sr"]
    _, w_kept, w_dt, w_parse = fx["one_call"]()
    with StoreBuilder(sr.filters, sr.txp_len) as b:
        kept_h = b.add_groups(fx["rec"][w_parse.order], w_parse.group_off)
        want, dt_h = b.export(), b.discard_table()
    assert np.array_equal(kept_h, w_kept) and dt_h == w_dt
    with _lib.testing() as L, RecordsStream(sr.filters, sr.txp_len, coverage=coverage, names=True) as s:
        for r, nm in fx["batches"]:
            s.push(r, names=nm)
        (rp, tid, p, st, en, sd, kept, dt), join_ms = finish_csr(L, s, coverage)
        info = s.info()
    assert join_ms > 0 and np.array_equal(kept, w_kept) and dt == w_dt
    assert np.array_equal(rp.astype(np.uint64), want[0]) and np.array_equal(tid, want[1])
    assert np.array_equal(p, want[2].view(np.uint32))
    if coverage is None:
        assert st is None
    else:
        assert np.array_equal(st, want[3]) and np.array_equal(en, want[4]) and np.array_equal(sd, want[5])
    assert info["batches"] == len(fx["batches"]) and info["records"] == len(fx["rec"]) and info["groups"] == len(w_kept)
    assert info["host_batches"] == 0


# ---- 3: the store ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coverage,coding,layout_build", [(None, 0, 0), ("logistic", 0, 0), ("binomial", 0, 0), (None, 2, 1)])
def test_the_store_is_the_one_calls(fx, coverage, coding, layout_build, monkeypatch):
    sr = fx["sr"]
    kw = dict(weight_coding=coding, layout_build=layout_build)
    monkeypatch.setenv("OEM_KEEP_UNPACKED", "1")                        # (oem_debug_layout_hash reads the builders' streams)
    with _lib.testing():
        got = session(sr.filters, sr.txp_len, fx["batches"], coverage=coverage, finish=kw)
        long, w_kept, w_dt, w_parse = DeviceStore.from_named_records(sr.filters, sr.txp_len, fx["rec"], fx["names"], mode="adjacent",
                                                                     coverage=coverage, **kw)
        with got[0] as one, long:
            same_outputs(got, (long, w_kept, w_dt, w_parse))
            assert one.n_reads == 20_000 and got[3].n_checked == w_parse.n_groups
            rows = [n.decode() for n in names_list(got[3].read_names)]
            _compare(one, long, fx["T"], coverage, rows)
            if coverage is None:
                assert _hash(one) == _hash(long)


# ---- 4: a read across many batches ----------------------------------------------------------------------------------
def test_a_read_of_300_records_pushed_one_record_per_batch():
    n_long, n_tail = 300, 40
    nl = [b"the-long-read"] * n_long + [b"read-%03d" % (i // 2) for i in range(n_tail)]
    rec = simple_records(n_long + n_tail)
    empty = (np.zeros(0, dtype=ALN_RECORD), pack([]))
    batches = []
    for i in range(n_long):
        batches.append((rec[i:i + 1], pack(nl[i:i + 1])))
        if i % 50 == 49:
            batches.append(empty)
    batches.append((rec[n_long:], pack(nl[n_long:])))
    k = len(batches) - n_long
    assert k == 7
    want = DeviceStore.from_named_records(FILTERS, TL, rec, pack(nl), mode="adjacent")
    got = session(FILTERS, TL, batches)
    with got[0], want[0]:
        same_outputs(got, want)
        assert got[3].group_off[1] == n_long and got[3].n_groups == 1 + n_tail // 2
        assert got[4]["batches"] == n_long + k and got[4]["records"] == n_long + n_tail
        assert (got[0].n_reads, got[0].nnz) == (want[0].n_reads, want[0].nnz)
        for a, b in zip(got[0].aux_counts(), want[0].aux_counts()):
            assert np.array_equal(a, b)


# ---- 5: the collation check -----------------------------------------------------------------------------------------
REPEAT = re.compile(r"group (\d+) \(first record (\d+)\).*\(first record (\d+)\)")


def one_call_repeat(nl, check):
    with pytest.raises(_lib.OemError) as ei:
        DeviceStore.from_named_records(FILTERS, TL, simple_records(len(nl)), pack(nl), mode="adjacent", sort_check_num=check)
    assert ei.value.code == _lib.OEM_ERR_STATE
    return REPEAT.search(str(ei.value)).groups()


@pytest.mark.parametrize("nl,cuts,repeat", [([b"A", b"B", b"A"], [2], ("2", "2", "0")),
                                            ([b"A", b"B", b"A", b"A"], [3], ("2", "2", "0")),      # the repeating group straddles the cut
                                            ([b"A", b"A", b"B", b"A"], [1], ("2", "3", "0"))])     # ... and so does the earlier one
def test_the_collation_check_covers_the_sessions_first_groups(nl, cuts, repeat):
    rec = simple_records(len(nl))
    batches = synth.cut_named_records(rec, pack(nl), cuts)
    assert one_call_repeat(nl, 3) == repeat
    with pytest.raises(_lib.OemError) as ei:
        session(FILTERS, TL, batches, check=3)
    assert ei.value.code == _lib.OEM_ERR_STATE and "not name-collated" in str(ei.value) and "OEM_COLLATE_SORT" in str(ei.value)
    assert REPEAT.search(str(ei.value)).groups() == repeat
    for check, n_checked in ((2, 2), (0, 0)):                            # a repeat at group N is accepted; N = 0 is no check
        want = DeviceStore.from_named_records(FILTERS, TL, rec, pack(nl), mode="adjacent", sort_check_num=check)
        got = session(FILTERS, TL, batches, check=check)
        with got[0], want[0]:
            same_outputs(got, want)
            assert got[3].n_checked == n_checked and got[3].n_groups == 3


def test_the_check_runs_once_n_groups_are_held_and_is_sticky_or_at_finish():
    nl = [b"A", b"B", b"A", b"C", b"D", b"E"]
    rec = simple_records(len(nl))
    batches = synth.cut_named_records(rec, pack(nl), [3, 4, 5])
    want = one_call_repeat(nl, 3)
    assert want == ("2", "2", "0")
    with RecordsStream(FILTERS, TL, names=True, sort_check_num=3, max_staged_records=1) as s:   # one batch at a time
        s.push(*batches[0][:1], names=batches[0][1])                     # closes A and B
        s.push(*batches[1][:1], names=batches[1][1])                     # C closes the second A: three heads are held
        for r, nm in batches[2:]:                                        # the next push waits for that batch: the sticky status
            with pytest.raises(_lib.OemError) as ei:
                s.push(r, names=nm)
            assert ei.value.code == _lib.OEM_ERR_STATE and REPEAT.search(str(ei.value)).groups() == want
        with pytest.raises(_lib.OemError) as ei:
            s.finish()
        assert ei.value.code == _lib.OEM_ERR_STATE and REPEAT.search(str(ei.value)).groups() == want
        assert s.info()["batches"] == 2
    # fewer than N groups: the check runs at finish
    with RecordsStream(FILTERS, TL, names=True, sort_check_num=10, max_staged_records=1) as s:
        for r, nm in batches:
            s.push(r, names=nm)
        with pytest.raises(_lib.OemError) as ei:
            s.finish()
        assert ei.value.code == _lib.OEM_ERR_STATE and REPEAT.search(str(ei.value)).groups() == one_call_repeat(nl, 10)
    ok = [b"A", b"B", b"C"]
    got = session(FILTERS, TL, synth.cut_named_records(simple_records(3), pack(ok), [1, 2]), check=10)
    with got[0]:
        assert got[3].n_checked == got[3].n_groups == 3


# ---- 6: threads -----------------------------------------------------------------------------------------------------
def test_four_threads_push_and_the_tickets_give_the_order(fx):
    sr = fx["sr"]
    n = len(fx["rec"])
    batches = synth.cut_named_records(fx["rec"], fx["names"], [(k * n) // 32 for k in range(1, 32)])
    assert len(batches) == 32
    tickets, errors = [None] * 32, []
    with RecordsStream(sr.filters, sr.txp_len, names=True, sort_check_num=0) as s:
        def pusher(t):
            try:
                for k in range(t, 32, 4):
                    tickets[k] = s.push(batches[k][0], names=batches[k][1])
            except Exception as e:                                      # noqa: BLE001
                errors.append(e)
        threads = [threading.Thread(target=pusher, args=(t,)) for t in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(JOIN_TIMEOUT)
        assert not any(t.is_alive() for t in threads) and not errors, errors
        assert sorted(tickets) == list(range(32))
        got = s.finish()
    rec, names = concat([batches[k] for k in np.argsort(tickets)])
    want = DeviceStore.from_named_records(sr.filters, sr.txp_len, rec, names, mode="adjacent", sort_check_num=0)
    with got[0] as one, want[0] as long:
        same_outputs(got, want)
        assert got[3].n_checked == 0 and one.n_reads >= 20_000
        _compare(one, long, fx["T"], None, [nm.decode() for nm in names_list(got[3].read_names)])


# ---- 7: errors and fallbacks ----------------------------------------------------------------------------------------
def pairs(n):
    return [b"read-%03d" % (i // 2) for i in range(n)]


@pytest.mark.parametrize("bad,word", [(b"", "record 30 has an empty name"), (b"AC\0G", "the name of record 30 contains a 0 byte")])
def test_a_bad_name_in_the_third_batch_carries_the_session_global_index(bad, word):
    nl = pairs(40)
    nl[30] = bad
    nl[35] = b""                                                        # a later one is not the one named
    unm = np.zeros(40, bool)
    unm[[3, 28]] = True
    batches = synth.cut_named_records(simple_records(40, unm), pack(nl), [13, 26])
    with pytest.raises(_lib.OemError) as ei:
        session(FILTERS, TL, batches)
    assert ei.value.code == _lib.OEM_ERR_ARG and word in str(ei.value), str(ei.value)
    nl[30], nl[35] = b"read-015", b"read-017"                            # the same bad name on an unmapped record is never read
    nl[28] = bad
    got = session(FILTERS, TL, synth.cut_named_records(simple_records(40, unm), pack(nl), [13, 26]))
    with got[0]:
        assert got[3].n_unmapped == 2 and got[3].n_groups == 20


@pytest.mark.parametrize("at,ticket", [(30, 2), (25, 1)])               # in a closed group; in the run its batch carries on
def test_a_bad_ref_id_carries_the_ticket_and_the_session_global_index(at, ticket):
    rec = simple_records(40)
    rec["ref_id"][at] = T
    rec["ref_id"][37] = T + 4                                           # a later one is not the one named
    batches = synth.cut_named_records(rec, pack(pairs(40)), [13, 26])
    with RecordsStream(FILTERS, TL, names=True, max_staged_records=1) as s:
        with pytest.raises(_lib.OemError) as ei:
            for r, nm in batches:
                s.push(r, names=nm)
            s.finish()
        msg = str(ei.value)
        assert ei.value.code == _lib.OEM_ERR_ARG and f"ticket {ticket}:" in msg and f"record {at}: ref_id {T} " in msg, msg
        with pytest.raises(_lib.OemError) as again:                      # sticky
            s.finish()
        assert again.value.code == _lib.OEM_ERR_ARG and f"record {at}:" in str(again.value)


def test_a_big_score_sends_its_batch_and_a_zero_denominator_every_batch_through_the_host_loop():
    n = 600
    unm = np.arange(n) % 13 == 4
    nl = pairs(n)
    big = simple_records(n, unm)
    big["score"][[300, 301]] = [2 ** 24 + 1, 2 ** 24 - 3]
    for F, rec, hosts in ((FILTERS, big, 1), (dict(FILTERS, score_prob_denom=0.0), simple_records(n, unm), None)):
        batches = synth.cut_named_records(rec, pack(nl), [151, 295, 449])      # 295 and 449 lie inside a read
        want = DeviceStore.from_named_records(F, TL, rec, pack(nl), mode="adjacent")
        got = session(F, TL, batches)
        with got[0], want[0]:
            same_outputs(got, want)
            assert (got[0].n_reads, got[0].nnz) == (want[0].n_reads, want[0].nnz) and got[0].n_reads > 250
            for a, b in zip(got[0].aux_counts(), want[0].aux_counts()):
                assert np.array_equal(a, b)
            if hosts is None:
                assert got[4]["host_batches"] == len(batches) + 1        # every batch closes groups, and finish the last one
            else:
                assert got[4]["host_batches"] == hosts


def test_back_pressure_empty_sessions_unmapped_only_and_destroy_with_staged_batches(fx):
    sr = fx["sr"]
    n = len(fx["rec"])
    batches = synth.cut_named_records(fx["rec"], fx["names"], [n // 3, 2 * n // 3])
    done = []
    with RecordsStream(sr.filters, sr.txp_len, names=True, max_staged_records=10) as s:      # a budget below any batch
        t = threading.Thread(target=lambda: done.append([s.push(r, names=nm) for r, nm in batches]))
        t.start()
        t.join(JOIN_TIMEOUT)
        assert not t.is_alive() and done == [[0, 1, 2]]
        got = s.finish() + (s.info(),)
    with got[0]:
        same_outputs(got, fx["one_call"]())
        assert got[4]["batches_before_finish"] >= 2
    got = session(sr.filters, sr.txp_len, [])                           # no batch at all
    with got[0] as one:
        assert (one.n_reads, one.nnz, one.n_txps) == (0, 0, fx["T"]) and len(got[1]) == 0 and sum(got[2].values()) == 0
        assert got[3].n_groups == 0 and list(got[3].group_off) == [0] and list(got[3].read_names[1]) == [0]
    for coverage in (None, "logistic"):                                 # unmapped records only, in two batches and an empty one
        b = (simple_records(3, [1, 1, 1]), pack([b"", b"a\0", b"zz"]))
        got = session(FILTERS, TL, [b, (np.zeros(0, dtype=ALN_RECORD), pack([])), b], coverage=coverage)
        with got[0] as one:
            assert (one.n_reads, one.nnz) == (0, 0) and got[3].n_groups == 0 and got[3].n_unmapped == 6 and got[3].n_parsed == 0
            assert sum(got[2].values()) == 0 and got[4]["batches"] == 3
    s = RecordsStream(sr.filters, sr.txp_len, names=True)               # destroyed with batches staged: returns
    for r, nm in batches:
        s.push(r, names=nm)
    t = threading.Thread(target=s.close)
    t.start()
    t.join(JOIN_TIMEOUT)
    assert not t.is_alive()


# ---- 8: the bulk driver ---------------------------------------------------------------------------------------------
def test_the_bulk_driver_from_record_batches_writes_the_files_of_the_one_from_records(fx, tmp_path):
    from oarfish_amd.bulk import BulkArgs, quantify_bulk_alignments_from_record_batches, quantify_bulk_alignments_from_records
    sr = fx["sr"]
    n = len(fx["rec"])
    txps = [f"ENST{i:011d}.{i % 13}" for i in range(fx["T"])]
    lens = [int(x) for x in sr.txp_len]
    batches = synth.cut_named_records(fx["rec"], fx["names"], [(k * n) // 5 for k in range(1, 5)])
    assert len(batches) == 5
    outs = [str(tmp_path / d / "sample") for d in ("batches", "whole")]
    args = [BulkArgs(output=o, write_assignment_probs=True, display_thresh=1e-4) for o in outs]
    got = quantify_bulk_alignments_from_record_batches(sr.filters, txps, lens, iter(batches), args[0])
    want = quantify_bulk_alignments_from_records(sr.filters, txps, lens, fx["rec"], fx["names"], args[1])
    # Two EM runs on one store differ in the last bits (f64 atomics: the one-call driver against ITSELF, three runs each
    # way on this input, differed by 3.9e-15 .. 8.3e-15 relative, the batches driver against it by no more), so the files
    # that print the counts are compared as tests/test_records_names_gpu.py compares them: the counts within its
    # tolerance, the files that do not depend on them byte for byte between the two drivers, and `.quant` / `.prob` byte
    # for byte against the one-call side's store, rows and names with the SAME counts put in.
    assert_counts_close(got, want, 20_000, fx["T"], rtol=1e-10, what="the driver from batches against the driver from records")
    assert open(outs[0] + ".ambig_info.tsv", "rb").read() == open(outs[1] + ".ambig_info.tsv", "rb").read()
    name_col = lambda path: [ln.split(b"\t")[0] for ln in open(path, "rb").read().split(b"\n")[fx["T"] + 1:]]   # noqa: E731
    assert name_col(outs[0] + ".prob") == name_col(outs[1] + ".prob") and len(name_col(outs[0] + ".prob")) == 20_000 + 1
    if np.array_equal(got, want):
        for ext in (".quant", ".prob"):
            assert open(outs[0] + ext, "rb").read() == open(outs[1] + ext, "rb").read(), ext
    long, _, _, parse = fx["one_call"]()
    with StoreBuilder(sr.filters, sr.txp_len) as hb:
        hb.add_groups(fx["rec"][parse.order], parse.group_off)
        row_ptr, tid = hb.export()[:2]
    rnames = [nm.decode() for nm in names_list(parse.read_names)]
    same = str(tmp_path / "same" / "sample")
    writers.write_output(same, {}, txps, lens, got, *long.aux_counts())
    writers.write_out_prob(same, row_ptr, tid, long.assignment_probs(got, 1e-4), rnames, txps, 1e-4)
    for ext in (".quant", ".ambig_info.tsv", ".prob"):
        a, b = open(outs[0] + ext, "rb").read(), open(same + ext, "rb").read()
        assert a == b and len(a) > 1000, ext
