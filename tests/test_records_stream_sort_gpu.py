"""GPU tests of the sorting names session (oem_records_stream_set_sort / _push_sort / _order_copy,
``RecordsStream(names=True, mode="sort")``, ``bulk.quantify_bulk_alignments_from_record_batches(mode="sort")``): in
whatever order the records come and wherever they are cut into batches, finish gives what
oem_store_create_records_names gives under OEM_COLLATE_SORT on the batches concatenated in ticket order -- order (as
64-bit session-global indices), group_off, kept, the discard table, every parse field, the row names and the store.
Everything is compared for equality."""
import ctypes as C
import threading

import numpy as np
import pytest

from oarfish_amd import _lib, synth
from oarfish_amd.builder import ALN_RECORD, RecordsStream
from oarfish_amd.types import DeviceStore

from tests.common import assert_counts_close
from tests.records_stream_names_common import T, U, cuttings16
from tests.records_stream_sort_common import names_list, sort_records16, sort_rule
from tests.test_filter_groups_gpu import _compare
from tests.test_records_stream_gpu import JOIN_TIMEOUT, _hash
from tests.test_records_stream_names_gpu import FILTERS, PARSE_FIELDS, TL, pack, simple_records

pytestmark = pytest.mark.gpu

EMPTY = (np.zeros(0, dtype=ALN_RECORD), pack([]), np.zeros(0, dtype=np.uint8))


def concat(batches):
    """(records, names, secondary) of the batches in this order; a batch without flags counts as flags of 0"""
    rec = np.concatenate([b[0] for b in batches]) if batches else np.zeros(0, dtype=ALN_RECORD)
    nl = [nm for b in batches for nm in names_list(b[1])]
    sec = [np.asarray(b[2], dtype=np.uint8) if len(b) > 2 and b[2] is not None else np.zeros(len(b[0]), dtype=np.uint8) for b in batches]
    return rec, pack(nl), (np.concatenate(sec) if sec else np.zeros(0, dtype=np.uint8))


def one_call(F, tl, rec, names, sec, coverage=None, **kw):
    return DeviceStore.from_named_records(F, tl, rec, names, secondary=sec, mode="sort", sort_check_num=0, coverage=coverage, **kw)


def session(F, tl, batches, coverage=None, finish=None, **kw):
    """(store, kept, dt, parse, info) of a sorting names session over the batches"""
    with RecordsStream(F, tl, coverage=coverage, names=True, mode="sort", **kw) as s:
        tickets = [s.push(b[0], names=b[1], secondary=b[2] if len(b) > 2 else None) for b in batches]
        assert tickets == list(range(len(batches)))
        store, kept, dt, parse = s.finish(**(finish or {}))
        return store, kept, dt, parse, s.info()


def same_outputs(got, want):
    """order, group_off, kept, the discard table, every parse field and the row names"""
    (_, kept, dt, parse), (_, w_kept, w_dt, w_parse) = got[:4], want[:4]
    assert parse.order.dtype == np.int64 and np.array_equal(parse.order, w_parse.order.astype(np.int64))
    assert np.array_equal(parse.group_off, w_parse.group_off) and parse.group_off.dtype == np.uint64
    assert np.array_equal(kept, w_kept) and dt == w_dt
    for f in PARSE_FIELDS:
        assert getattr(parse, f) == getattr(w_parse, f), f
    assert parse.n_checked == 0
    assert np.array_equal(parse.read_names[1], w_parse.read_names[1]) and np.array_equal(parse.read_names[0], w_parse.read_names[0])
    if len(got) > 4:
        assert got[4]["row_name_bytes"] == len(parse.read_names[0]) and got[4]["groups"] == w_parse.n_groups


def same_small_store(one, long):
    """dims, aux counts and, the testing library loaded, the packed layout's streams (CSR and weights) word for word"""
    assert (one.n_reads, one.nnz, one.n_txps) == (long.n_reads, long.nnz, long.n_txps)
    for a, b in zip(one.aux_counts(), long.aux_counts()):
        assert np.array_equal(a, b)
    assert _hash(one) == _hash(long)


def held(F, tl, batches, **kw):
    """the session over the batches against the one call on their concatenation: outputs and store"""
    want = one_call(F, tl, *concat(batches), **kw)
    got = session(F, tl, batches, **kw)
    with got[0] as one, want[0] as long:
        same_outputs(got, want)
        same_small_store(one, long)
    return got, want


@pytest.fixture
def testing(monkeypatch):
    monkeypatch.setenv("OEM_KEEP_UNPACKED", "1")                        # (oem_debug_layout_hash reads the builders' streams)
    with _lib.testing():
        yield


# ---- 1: exhaustive cuts ---------------------------------------------------------------------------------------------
def test_every_cutting_of_the_permuted_16_record_input_gives_the_one_calls_outputs(testing):
    rec, names, sec = sort_records16()
    want = one_call(FILTERS, TL, rec, names, sec)
    w_store, w_kept, _, w_parse = want
    order, group_off = sort_rule(rec, names, sec)                       # the rule in plain Python
    assert np.array_equal(w_parse.order, order) and np.array_equal(w_parse.group_off, group_off)
    assert w_parse.n_unmapped == 5 and w_parse.n_groups == 5 and int(w_kept.sum()) == w_store.nnz
    nl = names_list(names)
    rows = [nl[order[int(group_off[g])]] for g in np.flatnonzero(w_kept)]
    assert names_list(w_parse.read_names) == rows and len(rows) == 5
    with w_store:
        cs = cuttings16()
        assert len(cs) == 17 + 136 + 1
        for cuts in cs:
            batches = synth.cut_named_records(rec, names, cuts, secondary=sec)
            got = session(FILTERS, TL, batches)
            with got[0] as store:
                same_outputs(got, want)
                same_small_store(store, w_store)
                assert got[4]["batches"] == len(cuts) + 1 and got[4]["records"] == 16 and got[4]["arena_bytes"] > 0, cuts
                assert got[4]["host_batches"] == 0


# ---- 2: reads scattered over batches ----------------------------------------------------------------------------------
def test_reads_in_three_batches_with_a_secondary_pushed_before_its_primary(testing):
    nl = [b"A", b"B", b"C", b"B", b"A", b"C", b"C", b"A", b"B"]          # every read has a record in each of the three batches
    sec = np.array([1, 0, 1, 1, 0, 1, 0, 1, 1], dtype=np.uint8)          # A's primary is record 4, C's record 6: secondaries come first
    rec = simple_records(9)
    rec["score"] = 1000 - np.arange(9) % 2
    batches = synth.cut_named_records(rec, pack(nl), [3, 6], secondary=sec)
    got, want = held(FILTERS, TL, batches)
    assert list(got[3].order) == [4, 0, 7, 1, 3, 8, 6, 2, 5] and list(got[3].group_off) == [0, 3, 6, 9]
    # flags change the order, and a batch pushed without flags counts as flags of 0
    plain = [b[:2] for b in batches]
    got0, _ = held(FILTERS, TL, plain)
    assert list(got0[3].order) == [0, 4, 7, 1, 3, 8, 2, 5, 6]
    mixed = [batches[0], plain[1], batches[2]]
    got1, _ = held(FILTERS, TL, mixed)
    assert list(got1[3].order) == [4, 0, 7, 1, 3, 8, 5, 6, 2] == list(sort_rule(*concat(mixed))[0])


# ---- 3: unmapped records ----------------------------------------------------------------------------------------------
def test_unmapped_records_inside_and_between_reads_half_with_empty_names(testing):
    n = 120
    rng = np.random.default_rng(31)
    nl = [b"read-%02d" % k for k in rng.integers(0, 25, size=n)]
    unm = np.zeros(n, bool)
    unm[rng.choice(n, size=30, replace=False)] = True
    for k, i in enumerate(np.flatnonzero(unm)):
        nl[i] = b"" if k % 2 else (b"a\0b" if k % 4 == 0 else nl[i])     # never read: empty, a 0 byte, or a read's own name
    sec = (rng.random(n) < 0.5).astype(np.uint8)
    rec = simple_records(n, unm)
    for cuts in ([40, 80], [1, 2, 3, 119], list(range(10, 120, 10))):
        got, _ = held(FILTERS, TL, synth.cut_named_records(rec, pack(nl), cuts, secondary=sec))
        assert got[3].n_unmapped == 30 and got[3].n_parsed == 90
        assert np.array_equal(got[3].order, sort_rule(rec, pack(nl), sec)[0])    # session-global: the unmapped records counted


# ---- 4: the small ends ------------------------------------------------------------------------------------------------
def test_an_empty_batch_an_unmapped_only_batch_a_session_with_no_survivor_and_a_single_record(testing):
    unmapped3 = (simple_records(3, [1, 1, 1]), pack([b"", b"a\0", b"zz"]), np.array([1, 0, 1], dtype=np.uint8))
    rec, names, sec = sort_records16()
    a, b = synth.cut_named_records(rec, names, [7], secondary=sec)
    got, _ = held(FILTERS, TL, [EMPTY, a, unmapped3, EMPTY, b, EMPTY])
    assert got[4]["batches"] == 6 and got[4]["records"] == 19 and got[3].n_unmapped == 8
    assert list(got[3].order) == [i + (3 if i >= 7 else 0) for i in sort_rule(rec, names, sec)[0]]
    for coverage in (None, "logistic"):                                 # no survivor at all
        for batches in ([], [EMPTY], [unmapped3, EMPTY, unmapped3]):
            want = one_call(FILTERS, TL, *concat(batches), coverage=coverage)
            got = session(FILTERS, TL, batches, coverage=coverage)
            with got[0] as one, want[0]:
                same_outputs(got, want)
                assert (one.n_reads, one.nnz, one.n_txps) == (0, 0, T) and len(got[1]) == 0 and sum(got[2].values()) == 0
                assert len(got[3].order) == 0 and list(got[3].group_off) == [0] and list(got[3].read_names[1]) == [0]
                assert got[3].n_unmapped == sum(len(x[0]) for x in batches) and got[4]["arena_bytes"] == 0
    one = (simple_records(1), pack([b"the-only-read"]), np.array([1], dtype=np.uint8))
    got, _ = held(FILTERS, TL, [unmapped3, one])
    assert list(got[3].order) == [3] and got[3].n_groups == 1 and got[0].n_txps == T


# ---- 5: several key rounds --------------------------------------------------------------------------------------------
def test_illumina_style_names_share_21_bytes_and_differ_in_length(testing):
    sr = synth.make_records(synth.make_store(300, 50, kbar=3.0, seed=521), seed=522)
    rec, names, sec = synth.make_named_records(sr, style="illumina", seed=523, shuffle=True)
    nl = names_list(names)
    assert len({nm[:21] for nm in nl}) == 1 and len({len(nm) for nm in nl}) >= 2 and max(map(len, nl)) > 32
    cuts = list(range(64, len(rec), 64))
    got, _ = held(sr.filters, sr.txp_len, synth.cut_named_records(rec, names, cuts, secondary=sec))
    mapped = {nm for nm, f in zip(nl, rec["flags"]) if not f & U}       # (a dropped read of unmapped records only is no group)
    assert got[3].n_groups == len(mapped) and np.array_equal(got[3].order, sort_rule(rec, names, sec)[0])


# ---- the fixture of 6, 7, 8 and 12: ~2 000 reads, permuted, a fifth more unmapped records ------------------------------
@pytest.fixture(scope="module")
def fx():
    sr = synth.make_records(synth.make_store(2_000, 200, kbar=1.5, seed=511), seed=512)
    rec, names, sec = synth.make_named_records(sr, seed=513, unmapped_rate=0.2, shuffle=True)
    one = {}

    def want(coverage=None, **kw):
        key = (coverage, tuple(sorted(kw.items())))
        if key not in one:
            one[key] = one_call(sr.filters, sr.txp_len, rec, names, sec, coverage=coverage, **kw)
        return one[key]
    yield dict(sr=sr, rec=rec, names=names, sec=sec, want=want, T=len(sr.txp_len))
    for store, *_ in one.values():
        store.close()


def in_batches_of(fx, size):
    return synth.cut_named_records(fx["rec"], fx["names"], list(range(size, len(fx["rec"]), size)), secondary=fx["sec"])


def test_the_fixture_is_permuted_and_has_unmapped_records_with_empty_names(fx):
    rec, nl = fx["rec"], names_list(fx["names"])
    unm = (rec["flags"] & U) != 0
    assert 1_900 <= fx["want"]()[3].n_groups <= 2_200 and 0.12 < unm.mean() < 0.2
    empty = np.array([len(nm) == 0 for nm in nl])
    assert 0.3 < empty[unm].mean() < 0.7 and not empty[~unm].any()
    mapped = [nm for nm, u in zip(nl, unm) if not u]
    assert sum(a == b for a, b in zip(mapped[1:], mapped[:-1])) < len(mapped) // 20      # not collated
    assert fx["sec"][~unm].any() and not fx["sec"][~unm].all()


# ---- 6: the cut does not matter ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1, 7, 257])
def test_batches_of_1_7_and_257_records(fx, size, testing):
    sr = fx["sr"]
    batches = in_batches_of(fx, size)
    assert len(batches) == -(-len(fx["rec"]) // size)
    got = session(sr.filters, sr.txp_len, batches)
    want = fx["want"]()
    with got[0] as one:
        same_outputs(got, want)
        assert got[4]["records"] == len(fx["rec"]) and got[4]["batches"] == len(batches)
        assert got[4]["arena_bytes"] >= got[3].n_parsed * (40 + 8 + 8 + 1 + 36)      # record, offset, index, flag, a 36-byte name
        long = one_call(sr.filters, sr.txp_len, fx["rec"], fx["names"], fx["sec"])[0]    # (under the testing library: hashable)
        with long:
            same_small_store(one, long)
            _compare(one, long, fx["T"], None, [nm.decode() for nm in names_list(got[3].read_names)])


# ---- 7: threads -------------------------------------------------------------------------------------------------------
def test_four_threads_push_and_the_tickets_give_the_order(fx):
    sr = fx["sr"]
    n = len(fx["rec"])
    batches = synth.cut_named_records(fx["rec"], fx["names"], [(k * n) // 32 for k in range(1, 32)], secondary=fx["sec"])
    tickets, errors = [None] * 32, []
    with RecordsStream(sr.filters, sr.txp_len, names=True, mode="sort") as s:
        def pusher(t):
            try:
                for k in range(t, 32, 4):
                    tickets[k] = s.push(batches[k][0], names=batches[k][1], secondary=batches[k][2])
            except Exception as e:                                      # noqa: BLE001
                errors.append(e)
        threads = [threading.Thread(target=pusher, args=(t,)) for t in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(JOIN_TIMEOUT)
        assert not any(t.is_alive() for t in threads) and not errors, errors
        assert sorted(tickets) == list(range(32))
        got = s.finish() + (s.info(),)
    want = one_call(sr.filters, sr.txp_len, *concat([batches[k] for k in np.argsort(tickets)]))
    with got[0] as one, want[0] as long:
        same_outputs(got, want)
        _compare(one, long, fx["T"], None, [nm.decode() for nm in names_list(got[3].read_names)])


# ---- 8: the store's options -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coverage,coding,layout_build",
                         [(None, c, lb) for c in (0, 1, 2) for lb in (0, 1)] + [("logistic", 0, 0), ("binomial", 0, 0), ("logistic", 2, 1)])
def test_the_store_is_the_one_calls_for_every_coding_layout_build_and_model(fx, coverage, coding, layout_build, testing):
    sr = fx["sr"]
    kw = dict(weight_coding=coding, layout_build=layout_build)
    got = session(sr.filters, sr.txp_len, in_batches_of(fx, 257), coverage=coverage, finish=kw)
    long, w_kept, w_dt, w_parse = one_call(sr.filters, sr.txp_len, fx["rec"], fx["names"], fx["sec"], coverage=coverage, **kw)
    with got[0] as one, long:
        same_outputs(got, (long, w_kept, w_dt, w_parse))
        _compare(one, long, fx["T"], coverage, [nm.decode() for nm in names_list(got[3].read_names)])
        if coverage is None:
            assert _hash(one) == _hash(long)


# ---- 9: the host loop -------------------------------------------------------------------------------------------------
def test_a_big_score_and_a_zero_denominator_send_the_groups_through_the_host_loop_once(testing):
    n = 600
    rng = np.random.default_rng(91)
    perm = rng.permutation(n)
    unm = (np.arange(n) % 13 == 4)[perm]
    nl = [b"read-%03d" % (i // 2) for i in perm]
    sec = (perm % 2).astype(np.uint8)
    big = simple_records(n, unm)
    big["score"][np.flatnonzero(~unm)[[300, 301]]] = [2 ** 24 + 1, 2 ** 24 - 3]
    for F, rec in ((FILTERS, big), (dict(FILTERS, score_prob_denom=0.0), simple_records(n, unm))):
        got, _ = held(F, TL, synth.cut_named_records(rec, pack(nl), [151, 295, 449], secondary=sec))
        assert got[4]["host_batches"] == 1 and got[0].n_txps == T and got[3].n_reads > 250


# ---- 10: sticky errors ------------------------------------------------------------------------------------------------
def pairs(n):
    return [b"read-%03d" % ((i * 7) % n // 2) for i in range(n)]


@pytest.mark.parametrize("bad,word", [(b"", "record 20 has an empty name"), (b"AC\0G", "the name of record 20 contains a 0 byte")])
def test_a_bad_name_in_the_second_of_three_batches_carries_the_session_global_index(bad, word):
    nl = pairs(40)
    nl[20] = bad
    nl[22], nl[35] = b"", b"x\0"                                        # later ones are not the one named
    unm = np.zeros(40, bool)
    unm[[3, 15]] = True
    batches = synth.cut_named_records(simple_records(40, unm), pack(nl), [13, 26], secondary=np.zeros(40, dtype=np.uint8))
    with RecordsStream(FILTERS, TL, names=True, mode="sort", max_staged_records=1) as s:
        with pytest.raises(_lib.OemError) as ei:
            for r, nm, sc in batches:
                s.push(r, names=nm, secondary=sc)
            s.finish()
        assert ei.value.code == _lib.OEM_ERR_ARG and word in str(ei.value), str(ei.value)
        for call in (lambda: s.push(*batches[2][:1], names=batches[2][1]), s.finish):    # sticky
            with pytest.raises(_lib.OemError) as again:
                call()
            assert again.value.code == _lib.OEM_ERR_ARG and word in str(again.value)
        assert s.info()["batches"] <= 3
    nl[20], nl[22], nl[35] = b"read-000", b"read-001", b"read-002"       # the same bad name on an unmapped record is never read
    nl[15] = bad
    got = session(FILTERS, TL, synth.cut_named_records(simple_records(40, unm), pack(nl), [13, 26]))
    with got[0]:
        assert got[3].n_unmapped == 2 and got[3].n_parsed == 38


def test_a_bad_ref_id_in_the_second_of_three_batches_carries_the_ticket_and_the_session_global_index():
    rec = simple_records(40)
    rec["ref_id"][20] = T
    rec["ref_id"][[24, 37]] = T + 4                                     # later ones are not the one named
    batches = synth.cut_named_records(rec, pack(pairs(40)), [13, 26])
    with RecordsStream(FILTERS, TL, names=True, mode="sort", max_staged_records=1) as s:
        with pytest.raises(_lib.OemError) as ei:
            for r, nm in batches:
                s.push(r, names=nm)
            s.finish()
        msg = str(ei.value)
        assert ei.value.code == _lib.OEM_ERR_ARG and "ticket 1:" in msg and f"record 20: ref_id {T} " in msg, msg
        with pytest.raises(_lib.OemError) as again:                      # sticky
            s.finish()
        assert again.value.code == _lib.OEM_ERR_ARG and "record 20:" in str(again.value)
    rec["flags"][[20, 24, 37]] = U                                      # an unmapped record's ref_id is never read
    got = session(FILTERS, TL, synth.cut_named_records(rec, pack(pairs(40)), [13, 26]))
    with got[0]:
        assert got[3].n_unmapped == 3


# ---- 11: the state errors ---------------------------------------------------------------------------------------------
def test_the_state_errors():
    L = _lib.lib()
    rec, names, sec = sort_records16()
    out = np.zeros(16, dtype=np.uint64)
    with RecordsStream(FILTERS, TL) as s:                               # set_sort after a push
        s.push(simple_records(2), np.array([0, 2], dtype=np.uint64))
        assert L.oem_records_stream_set_sort(s.handle) == _lib.OEM_ERR_STATE and b"pushed already" in L.oem_last_error()
    for kw in (dict(names=True), dict(projected=True)):                 # ... and after another set_*
        with RecordsStream(FILTERS, TL, **kw) as s:
            assert L.oem_records_stream_set_sort(s.handle) == _lib.OEM_ERR_STATE
            assert L.oem_records_stream_order_copy(s.handle, out.ctypes.data) == _lib.OEM_ERR_STATE
            with pytest.raises(_lib.OemError) as ei:
                t = C.c_uint64(0)
                s._check(L.oem_records_stream_push_sort(s.handle, rec.ctypes.data, 16, names[0].ctypes.data, names[1].ctypes.data,
                                                        sec.ctypes.data, C.byref(t)))
            assert ei.value.code == _lib.OEM_ERR_STATE and "not a sorting names session" in str(ei.value)
    with RecordsStream(FILTERS, TL, names=True, mode="sort") as s:
        assert L.oem_records_stream_order_copy(s.handle, out.ctypes.data) == _lib.OEM_ERR_STATE      # before finish
        s.push(rec, names=names, secondary=sec)
        store, _, _, parse = s.finish()
        store.close()
        assert L.oem_records_stream_set_sort(s.handle) == _lib.OEM_ERR_STATE                         # after finish
        with pytest.raises(_lib.OemError) as ei:
            s.push(rec, names=names, secondary=sec)
        assert ei.value.code == _lib.OEM_ERR_STATE
        with pytest.raises(_lib.OemError) as ei:
            s.finish()
        assert ei.value.code == _lib.OEM_ERR_STATE
        assert L.oem_records_stream_order_copy(s.handle, out.ctypes.data) == _lib.OEM_OK             # ... and again
        assert np.array_equal(out[:11].astype(np.int64), parse.order) and not out[11:].any()
        assert L.oem_records_stream_order_copy(s.handle, None) == _lib.OEM_ERR_ARG
    with _lib.testing() as Lt, RecordsStream(FILTERS, TL, names=True, mode="sort") as s:             # no joined CSR to show
        dims, caps = (C.c_uint64 * 3)(), (C.c_uint64 * 3)(0, 0, 0)
        assert Lt.oem_debug_records_stream_finish_csr(s.handle, dims, caps, None, None, None, None, None, None, None, None, None) == _lib.OEM_ERR_STATE


# ---- 12: the bulk driver ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob_on_device", [False, True])
def test_the_bulk_driver_in_sort_mode_writes_the_files_of_the_one_from_records(fx, tmp_path, prob_on_device):
    from oarfish_amd.bulk import BulkArgs, quantify_bulk_alignments_from_record_batches, quantify_bulk_alignments_from_records
    sr = fx["sr"]
    n = len(fx["rec"])
    txps = [f"ENST{i:011d}.{i % 13}" for i in range(fx["T"])]
    lens = [int(x) for x in sr.txp_len]
    batches = synth.cut_named_records(fx["rec"], fx["names"], [(k * n) // 5 for k in range(1, 5)], secondary=fx["sec"])
    outs = [str(tmp_path / d / "sample") for d in ("batches", "whole")]
    args = [BulkArgs(output=o, write_assignment_probs=True, display_thresh=1e-4, prob_on_device=prob_on_device) for o in outs]
    got = quantify_bulk_alignments_from_record_batches(sr.filters, txps, lens, iter(batches), args[0], mode="sort")
    want = quantify_bulk_alignments_from_records(sr.filters, txps, lens, fx["rec"], fx["names"], args[1], secondary=fx["sec"],
                                                 mode="sort")
    # Two EM runs on one store differ in the last bits (f64 atomics), so the files that print the counts are compared as
    # tests/test_records_stream_names_gpu.py compares them: the counts within its tolerance, the files that do not
    # depend on them byte for byte, and `.quant` / `.prob` byte for byte where the two runs gave the same counts.
    n_reads = fx["want"]()[3].n_reads
    assert_counts_close(got, want, n_reads, fx["T"], rtol=1e-10, what="the driver from batches against the driver from records")
    assert open(outs[0] + ".ambig_info.tsv", "rb").read() == open(outs[1] + ".ambig_info.tsv", "rb").read()
    name_col = lambda path: [ln.split(b"\t")[0] for ln in open(path, "rb").read().split(b"\n")[fx["T"] + 1:]]   # noqa: E731
    assert name_col(outs[0] + ".prob") == name_col(outs[1] + ".prob") and len(name_col(outs[0] + ".prob")) == n_reads + 1
    if np.array_equal(got, want):
        for ext in (".quant", ".prob"):
            assert open(outs[0] + ext, "rb").read() == open(outs[1] + ext, "rb").read(), ext
    with pytest.raises(ValueError, match="a batch is"):
        quantify_bulk_alignments_from_record_batches(sr.filters, txps, lens, iter([batches[0]]), args[0])   # flags without mode="sort"
