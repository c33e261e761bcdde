"""GPU tests of the bulk records session (oem_records_stream_*, oem_records_stream.hip): whatever way the records are cut
into batches and whichever thread pushes them, finish gives what oem_store_create_records gives on the batches
concatenated in ticket order -- the joined CSR bit for bit (k_stream_concat, through the test-only library's hook), the
store for every coverage model, weight coding and layout builder, under back-pressure, through the host-loop fallbacks
and around every error the session reports."""
import ctypes as C
import dataclasses
import threading

import numpy as np
import pytest

from oarfish_amd import _lib, synth
from oarfish_amd.builder import ALN_RECORD, RecordsStream, StoreBuilder
from oarfish_amd.types import DeviceStore
from oracle import filter_py as fp

from tests.filter_common import filters_dict, pack, random_groups
from tests.test_filter_groups_gpu import _compare

pytestmark = pytest.mark.gpu

JOIN_TIMEOUT = 120.0                                                    # a pushing thread still alive then: a deadlock


# ---- batches -------------------------------------------------------------------------------------------------------
def cut(records, group_off, sizes):
    """the groups cut at group boundaries into batches of these sizes (the last entry repeats until the end)"""
    out, g, k = [], 0, 0
    n = len(group_off) - 1
    while g < n or k < len(sizes) - 1:
        m = min(sizes[min(k, len(sizes) - 1)], n - g)
        r0, r1 = int(group_off[g]), int(group_off[g + m])
        out.append((records[r0:r1].copy(), (group_off[g:g + m + 1] - group_off[g]).astype(np.uint64)))
        g, k = g + m, k + 1
    return out


def concat(batches):
    rec = np.concatenate([b[0] for b in batches]) if batches else np.zeros(0, dtype=ALN_RECORD)
    off, base = [np.zeros(1, dtype=np.uint64)], 0
    for r, o in batches:
        off.append(o[1:] + np.uint64(base))
        base += len(r)
    return rec, np.concatenate(off)


SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 3001]


@pytest.fixture(scope="module")
def fx():
    """the fixture of tests/test_filter_groups_gpu.py, cut into batches with two planted ones, and the host builder's
    answer on the concatenation"""
    st = synth.make_store(20_000, 500, seed=411)
    sr = synth.make_records(st, seed=412)
    batches = cut(sr.records, sr.group_off, SIZES)
    empty = (np.zeros(0, dtype=ALN_RECORD), np.zeros(1, dtype=np.uint64))
    dropped = pack([[fp.Rec(0, 0, 0, 0, None, 100, unmapped=True)], [], [fp.Rec(1, 0, 0, 0, None, 90, unmapped=True)]])
    batches.insert(9, empty)                                            # between the 257 and the 1000
    batches.insert(12, dropped)                                         # a piece of zero rows between two pieces of 3001
    rec, off = concat(batches)
    b = StoreBuilder(sr.filters, sr.txp_len)
    kept = b.add_groups(rec, off)
    names = [f"read{g}/{g % 7}" for g in range(len(kept))]
    yield dict(sr=sr, batches=batches, rec=rec, off=off, builder=b, kept=kept, names=names, T=len(sr.txp_len))
    b.close()


def push_all(s, batches):
    return [s.push(r, o) for r, o in batches]


def finish_csr(L, s, model):
    """the session ended through the test-only hook: (row_ptr, tid, as_prob bits, start, end, strand, kept, discard)"""
    dims, caps = (C.c_uint64 * 3)(), (C.c_uint64 * 3)(1 << 22, 1 << 22, 1 << 22)
    n = 1 << 22
    rp, tid, p = np.zeros(n + 1, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    st, en, sd, kept = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    dt, ms = _lib.DiscardTableC(), C.c_float(-1.0)
    s._check(L.oem_debug_records_stream_finish_csr(s.handle, dims, caps, rp.ctypes.data, tid.ctypes.data, p.ctypes.data,
                                                   st.ctypes.data, en.ctypes.data, sd.ctypes.data, kept.ctypes.data,
                                                   C.addressof(dt), C.addressof(ms)))
    R, A, G = (int(x) for x in dims)
    from oarfish_amd.builder import discard_dict
    out = (rp[:R + 1], tid[:A], p[:A], st[:A], en[:A], sd[:A], kept[:G], discard_dict(dt))
    return out if model is not None else out[:3] + (None, None, None) + out[6:], float(ms.value)


def same_store(one, long, fx, coverage, got, want):
    """dims, kept and discard table, then tests/test_filter_groups_gpu.py's _compare"""
    (got_kept, got_dt), (want_kept, want_dt) = got, want
    assert np.array_equal(got_kept, want_kept) and got_dt == want_dt
    names_kept = [fx["names"][g] for g in np.flatnonzero(want_kept)] if fx is not None else \
                 [f"r{g}" for g in np.flatnonzero(want_kept)]
    return _compare(one, long, one.n_txps, coverage, names_kept)


def _hash(store):
    out = (C.c_uint64 * 18)()
    store._check(store._lib.oem_debug_layout_hash(store.handle, out, 18))
    return list(out)


# ---- 1: the join, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("coverage", [None, "logistic"])
def test_the_joined_csr_is_the_host_builders_bit_for_bit(fx, coverage):
    want = fx["builder"].export()
    sizes = np.array([len(o) - 1 for _, o in fx["batches"]])
    assert sizes[0] == 0 and sizes[9] == 0 and list(sizes[1:9]) == SIZES[1:9] and 3001 in sizes
    bases = np.concatenate([[0], np.cumsum(fx["kept"].astype(np.int64))])[np.cumsum(sizes)[:-1]]   # the pieces' alignment bases
    assert (bases % 2 == 1).any() and (bases % 4 != 0).any() and (bases % 16 != 0).any()          # the unaligned copy paths run
    kept_of = np.add.reduceat(np.append(fx["kept"], 0).astype(np.int64), np.minimum(np.cumsum(sizes) - sizes, len(fx["kept"])))
    assert kept_of[12] == 0 and sizes[12] == 3 and kept_of[11] > 0 and kept_of[13] > 0             # a piece of zero rows between two
    with _lib.testing() as L, RecordsStream(fx["sr"].filters, fx["sr"].txp_len, coverage=coverage) as s:
        assert push_all(s, fx["batches"]) == list(range(len(fx["batches"])))
        (rp, tid, p, st, en, sd, kept, dt), join_ms = finish_csr(L, s, coverage)
        info = s.info()
    assert join_ms > 0                                                  # the kernel ran
    assert np.array_equal(kept, fx["kept"]) and dt == fx["builder"].discard_table()
    assert np.array_equal(rp.astype(np.uint64), want[0]) and np.array_equal(tid, want[1])
    assert np.array_equal(p, want[2].view(np.uint32))
    if coverage is None:
        assert st is None
    else:
        assert np.array_equal(st, want[3]) and np.array_equal(en, want[4]) and np.array_equal(sd, want[5])
    assert info["batches"] == len(fx["batches"]) and info["groups"] == len(fx["kept"]) and info["records"] == len(fx["rec"])
    assert info["host_batches"] == 0


def test_the_joined_csr_of_both_strands_at_odd_bases():
    """the fixture above keeps forward alignments only (its strand column is all 0): random groups of both strands, cut
    small, so that the byte column is joined at bases of every residue mod 4 with something to get wrong"""
    F, txp_len, groups = random_groups(31, 4000, T=120)
    F = filters_dict(dataclasses.replace(F, which_strand=0, three_prime_clip=2 ** 62))
    rec, off = pack(groups)
    batches = cut(rec, off, [1, 2, 3, 63, 65, 255, 257, 1000, 511])
    with StoreBuilder(F, txp_len) as b:
        want_kept = b.add_groups(rec, off)
        want, want_dt = b.export(), b.discard_table()
    sizes = np.array([len(o) - 1 for _, o in batches])
    bases = np.concatenate([[0], np.cumsum(want_kept.astype(np.int64))])[np.cumsum(sizes)[:-1]]
    assert set(bases % 4) == {0, 1, 2, 3} and len(batches) >= 12
    with _lib.testing() as L, RecordsStream(F, txp_len, coverage="binomial") as s:
        push_all(s, batches)
        (rp, tid, p, st, en, sd, kept, dt), join_ms = finish_csr(L, s, "binomial")
    assert join_ms > 0 and np.array_equal(kept, want_kept) and dt == want_dt
    assert np.array_equal(rp.astype(np.uint64), want[0]) and np.array_equal(tid, want[1]) and np.array_equal(p, want[2].view(np.uint32))
    assert np.array_equal(st, want[3]) and np.array_equal(en, want[4]) and np.array_equal(sd, want[5])
    assert len(sd) > 500 and 0.1 * len(sd) < sd.sum() < 0.9 * len(sd)


# ---- 2: the store ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout_build", [0, 1])
@pytest.mark.parametrize("coding", [0, 1, 2])
@pytest.mark.parametrize("coverage", [None, "logistic", "binomial"])
def test_the_store_is_the_one_calls(fx, coverage, coding, layout_build, monkeypatch):
    kw = dict(weight_coding=coding, layout_build=layout_build)
    monkeypatch.setenv("OEM_KEEP_UNPACKED", "1")                        # (oem_debug_layout_hash reads the builders' streams)
    with _lib.testing():
        with RecordsStream(fx["sr"].filters, fx["sr"].txp_len, coverage=coverage) as s:
            push_all(s, fx["batches"])
            one, kept, dt = s.finish(**kw)
        long, want_kept, want_dt = DeviceStore.from_records(fx["sr"].filters, fx["sr"].txp_len, fx["rec"], fx["off"],
                                                            coverage=coverage, **kw)
        with one, long:
            assert np.array_equal(want_kept, fx["kept"]) and one.n_reads == 20_000
            same_store(one, long, fx, coverage, (kept, dt), (want_kept, want_dt))
            if coverage is None:
                assert _hash(one) == _hash(long)


# ---- 3: threads and tickets -----------------------------------------------------------------------------------------
def test_four_threads_push_and_the_tickets_give_the_order(fx):
    sr = fx["sr"]
    batches = cut(sr.records, sr.group_off, [(len(sr.group_off) - 1 + 31) // 32])
    assert len(batches) == 32
    tickets, errors = [None] * 32, []
    with RecordsStream(sr.filters, sr.txp_len, coverage="logistic") as s:
        def pusher(t):
            try:
                for k in range(t, 32, 4):
                    tickets[k] = s.push(*batches[k])
            except Exception as e:                                      # noqa: BLE001
                errors.append(e)
        threads = [threading.Thread(target=pusher, args=(t,)) for t in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(JOIN_TIMEOUT)
        assert not any(t.is_alive() for t in threads) and not errors, errors
        assert sorted(tickets) == list(range(32))
        one, kept, dt = s.finish()
    order = np.argsort(tickets)
    rec, off = concat([batches[k] for k in order])
    long, want_kept, want_dt = DeviceStore.from_records(sr.filters, sr.txp_len, rec, off, coverage="logistic")
    with one, long:
        same_store(one, long, None, "logistic", (kept, dt), (want_kept, want_dt))


# ---- 4: back-pressure -----------------------------------------------------------------------------------------------
def test_back_pressure_admits_a_batch_once_its_predecessor_has_left_the_staging(fx):
    sr = fx["sr"]
    batches = cut(sr.records, sr.group_off, [(len(sr.group_off) - 1 + 5) // 6])
    assert len(batches) == 6
    n = [len(r) for r, _ in batches]
    budget = min(a + b for a, b in zip(n, n[1:])) - 1                   # below any two neighbours: one batch at a time
    assert budget > max(n)
    done = []
    with RecordsStream(sr.filters, sr.txp_len, max_staged_records=budget) as s:
        t = threading.Thread(target=lambda: done.append(push_all(s, batches)))
        t.start()
        t.join(JOIN_TIMEOUT)
        assert not t.is_alive() and done == [list(range(6))]
        before = s.info()["batches_before_finish"]
        one, kept, dt = s.finish()
        info = s.info()
    assert before >= 5 and info["batches_before_finish"] >= 5
    long, want_kept, want_dt = DeviceStore.from_records(sr.filters, sr.txp_len, sr.records, sr.group_off)
    with one, long:
        same_store(one, long, None, None, (kept, dt), (want_kept, want_dt))
    with RecordsStream(sr.filters, sr.txp_len, max_staged_records=10) as s:   # every batch is larger than the budget
        t = threading.Thread(target=lambda: done.append(push_all(s, batches[:3])))
        t.start()
        t.join(JOIN_TIMEOUT)
        assert not t.is_alive() and done[-1] == [0, 1, 2]
        one, kept, dt = s.finish()
        with one:
            assert np.array_equal(kept, want_kept[:len(kept)]) and one.n_reads == np.count_nonzero(kept)


# ---- 5: fallbacks ---------------------------------------------------------------------------------------------------
def test_a_big_score_sends_its_batch_and_a_zero_denominator_every_batch_through_the_host_loop():
    F, txp_len, groups = random_groups(31, 1500, T=120)
    F = dataclasses.replace(F, which_strand=0, three_prime_clip=2 ** 62)   # (the two planted records pass the predicate)
    groups = list(groups)
    groups[700] = [fp.Rec(3, 10, 900, 800, 2 ** 24 + 1, 900), fp.Rec(4, 10, 900, 800, 2 ** 24 - 3, None)]
    rec, off = pack(groups)
    batches = cut(rec, off, [300])
    with RecordsStream(filters_dict(F), txp_len) as s:
        push_all(s, batches)
        one, kept, dt = s.finish()
        assert s.info()["host_batches"] == 1 and s.info()["batches"] == 5
    long, want_kept, want_dt = DeviceStore.from_records(filters_dict(F), txp_len, rec, off)
    with one, long:
        assert kept[700] == 2
        same_store(one, long, None, None, (kept, dt), (want_kept, want_dt))
    F0 = filters_dict(dataclasses.replace(F, score_prob_denom=0.0))     # no table: the one call's result is the host loop's
    with StoreBuilder(F0, txp_len) as b:
        want_kept = b.add_groups(rec, off)
        want, want_dt = b.export(), b.discard_table()
    with _lib.testing() as L, RecordsStream(F0, txp_len, coverage="logistic") as s:
        push_all(s, batches)
        (rp, tid, p, st, en, sd, kept, dt), _ = finish_csr(L, s, "logistic")
        assert s.info()["host_batches"] == 5
    assert np.array_equal(kept, want_kept) and dt == want_dt and np.count_nonzero(kept) > 100
    assert np.array_equal(rp.astype(np.uint64), want[0]) and np.array_equal(tid, want[1])
    assert np.array_equal(p, want[2].view(np.uint32)) and np.all(np.isnan(want[2]) | (want[2] == 0))   # 0/0 and -g/0
    assert np.array_equal(st, want[3]) and np.array_equal(en, want[4]) and np.array_equal(sd, want[5])


# ---- 6: errors ------------------------------------------------------------------------------------------------------
def test_a_rejected_batch_uses_no_ticket_and_leaves_the_session_usable(fx):
    sr = fx["sr"]
    batches = cut(sr.records, sr.group_off, [4000])
    with RecordsStream(sr.filters, sr.txp_len) as s:
        assert s.push(*batches[0]) == 0
        bad = batches[1][1].copy()
        bad[9] = bad[10] + 1
        with pytest.raises(_lib.OemError) as ei:
            s.push(batches[1][0], bad)
        assert ei.value.code == _lib.OEM_ERR_ARG and "decreases" in str(ei.value)
        assert s.push(*batches[2]) == 1 and s.info()["batches"] == 2
        one, kept, dt = s.finish()
    rec, off = concat([batches[0], batches[2]])
    long, want_kept, want_dt = DeviceStore.from_records(sr.filters, sr.txp_len, rec, off)
    with one, long:
        same_store(one, long, None, None, (kept, dt), (want_kept, want_dt))


def test_a_bad_ref_id_is_sticky_and_names_ticket_and_record(fx):
    sr = fx["sr"]
    batches = cut(sr.records, sr.group_off, [(len(sr.group_off) - 1 + 5) // 6])
    r2 = batches[2][0].copy()
    at = int(np.flatnonzero((r2["flags"] & _lib.REC_UNMAPPED) == 0)[40])
    r2["ref_id"][at] = fx["T"]
    later = at + 1 + int(np.flatnonzero((r2["flags"][at + 1:] & _lib.REC_UNMAPPED) == 0)[100])
    r2["ref_id"][later] = fx["T"] + 5                                   # a later one: not the one named
    n = max(len(r) for r, _ in batches)
    with RecordsStream(sr.filters, sr.txp_len, max_staged_records=n) as s:   # one batch at a time: push 3 sees batch 2's end
        assert [s.push(*batches[0]), s.push(*batches[1]), s.push(r2, batches[2][1])] == [0, 1, 2]
        for k in (3, 4, 5):
            with pytest.raises(_lib.OemError) as ei:
                s.push(*batches[k])
            assert ei.value.code == _lib.OEM_ERR_ARG
            assert "ticket 2:" in str(ei.value) and f"record {at}:" in str(ei.value) and f"ref_id {fx['T']} " in str(ei.value)
        h = C.c_void_p(1)
        assert s._lib.oem_records_stream_finish(s.handle, None, None, None, C.byref(h)) == _lib.OEM_ERR_ARG and not h.value
        assert b"ticket 2:" in s._lib.oem_last_error()


def test_state_errors_empty_sessions_and_destroy_with_staged_batches(fx):
    sr = fx["sr"]
    batches = cut(sr.records, sr.group_off, [5000])
    with RecordsStream(sr.filters, sr.txp_len) as s:                    # no batches at all
        one, kept, dt = s.finish()
        with one:
            assert (one.n_reads, one.nnz, one.n_txps) == (0, 0, fx["T"]) and len(kept) == 0 and sum(dt.values()) == 0
        with pytest.raises(_lib.OemError) as ei:
            s.push(*batches[0])
        assert ei.value.code == _lib.OEM_ERR_STATE
        h = C.c_void_p(1)
        assert s._lib.oem_records_stream_finish(s.handle, None, None, None, C.byref(h)) == _lib.OEM_ERR_STATE and not h.value
    dropped = pack([[fp.Rec(0, 0, 0, 0, None, 100, unmapped=True)], [], [fp.Rec(1, 10, 900, 800, 0, 900)]])
    for coverage in (None, "logistic"):
        with RecordsStream(sr.filters, sr.txp_len, coverage=coverage) as s:   # dropped reads only, in two batches
            s.push(*dropped)
            s.push(*dropped)
            one, kept, dt = s.finish()
            with one:
                assert (one.n_reads, one.nnz) == (0, 0) and list(kept) == [0] * 6 and dt["no_mapping"] == dt["no_valid_aln"] == 2
    with RecordsStream(sr.filters, sr.txp_len) as s:                    # a bad option is reported before the session ends
        s.push(*batches[0])
        with pytest.raises(_lib.OemError) as ei:
            s.finish(weight_coding=3)
        assert ei.value.code == _lib.OEM_ERR_ARG
        one, kept, dt = s.finish()
        with one:
            assert one.n_reads == np.count_nonzero(kept) > 0
    s = RecordsStream(sr.filters, sr.txp_len)                           # destroyed with batches staged: returns
    push_all(s, batches)
    t = threading.Thread(target=s.close)
    t.start()
    t.join(JOIN_TIMEOUT)
    assert not t.is_alive()


# ---- 7: Python ------------------------------------------------------------------------------------------------------
def test_records_stream_returns_from_records_triple():
    F, txp_len, groups = random_groups(7, 900, T=60)
    F = dataclasses.replace(F, which_strand=0, three_prime_clip=2 ** 62)
    rec, off = pack(groups)
    with RecordsStream(filters_dict(F), txp_len) as s:
        assert [s.push(*b) for b in cut(rec, off, [250])] == [0, 1, 2, 3]
        info = s.info()
        assert set(info) == {"batches", "groups", "records", "batches_before_finish", "blocked_us", "host_batches"}
        assert (info["batches"], info["groups"], info["records"]) == (4, 900, len(rec))
        one, kept, dt = s.finish()
    long, want_kept, want_dt = DeviceStore.from_records(filters_dict(F), txp_len, rec, off)
    with one, long:
        assert isinstance(one, DeviceStore) and kept.dtype == np.uint32 and isinstance(dt, dict)
        assert np.count_nonzero(kept) > 100
        same_store(one, long, None, None, (kept, dt), (want_kept, want_dt))
