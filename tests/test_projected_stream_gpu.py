"""GPU tests of the projected session (oem_records_stream_set_projected / _push_projected, oem_records_stream.hip and
k_proj_collect of oem_filter_projected_device.hip): however the genome-mode groups are cut into batches and whichever
thread pushes them, finish gives what oem_store_create_projected_records gives on the batches concatenated in ticket
order -- kept, the discard table, the joined CSR with as_prob bit for bit, the store for every probability source and
coverage model -- with the deferred expf really exercised, through the host-loop fallbacks and around the sticky errors;
and the genome-mode bulk drivers write the files of the host path."""
import ctypes as C
import json
import math
import struct
import threading

import numpy as np
import pytest

from oarfish_amd import _lib, synth, writers
from oarfish_amd.builder import PROJ_RECORD, RecordsStream, StoreBuilder
from oarfish_amd.types import DeviceStore, InMemoryAlignmentStore
from oracle import filter_py as fp

from tests import projected_ref as pr
from tests.common import assert_counts_close
from tests.test_filter_groups_gpu import _compare
from tests.test_records_stream_gpu import JOIN_TIMEOUT, _hash, finish_csr

pytestmark = pytest.mark.gpu

f32 = np.float32
FLT_MIN = 1.17549435e-38
COVERAGES = [None, "logistic", "binomial"]


# ---- inputs ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spr():
    return synth.make_projected_records(synth.make_store(3000, 300, kbar=6))


def cuttings(G):
    """the issue's three: one batch; the edges of the 256-lane kernels and the 64-lane ballot; 40 single groups and the rest"""
    edges = [1, 0, 255, 256, 257, 64]
    return {"one": [G], "edges": edges + [G - sum(edges)], "forty": [1] * 40 + [G - 40]}


def concat(batches):
    rec = np.concatenate([b[0] for b in batches]) if batches else np.zeros(0, dtype=PROJ_RECORD)
    off, base = [np.zeros(1, dtype=np.uint64)], 0
    for r, o, _ in batches:
        off.append(o[1:] + np.uint64(base))
        base += len(r)
    rl = np.concatenate([b[2] for b in batches]) if batches else np.zeros(0, dtype=np.uint64)
    return rec, np.concatenate(off), rl


def push_all(s, batches):
    return [s.push(r, o, read_len=l) for r, o, l in batches]


def same_store(one, long, coverage, got, want):
    (got_kept, got_dt), (want_kept, want_dt) = got, want
    assert np.array_equal(got_kept, want_kept) and got_dt == want_dt
    return _compare(one, long, one.n_txps, coverage, [f"r{g}" for g in np.flatnonzero(want_kept)])


def host_answer(filters, txp_len, rec, off, rl, beta, source):
    """the host builder's arrays, kept and discard table on the concatenation"""
    with StoreBuilder(filters, txp_len) as b:
        kept = b.add_projected_groups(rec, off, rl, beta=beta, prob_source=source)
        return b.export(), kept, b.discard_table()


def csr_equals_host(got, want, kept, dt, coverage):
    rp, tid, p, st, en, sd, got_kept, got_dt = got
    arrays, want_kept, want_dt = want
    assert np.array_equal(got_kept, want_kept) and got_dt == want_dt
    assert np.array_equal(got_kept, kept) and got_dt == dt
    assert np.array_equal(rp.astype(np.uint64), arrays[0]) and np.array_equal(tid, arrays[1])
    assert np.array_equal(p, arrays[2].view(np.uint32))                 # as_prob bit for bit
    if coverage is not None:
        assert np.array_equal(st, arrays[3]) and np.array_equal(en, arrays[4]) and np.array_equal(sd, arrays[5])


# ---- the Python restatement of "sure" (oarfish_amd/csrc/oem_exp_f32.h) over tests/projected_ref.py's arithmetic ------
def is_sure(f):
    f = float(f32(f))
    if not (f <= 0.0) or f < -3.4028234663852886e38:                    # NaN, positive, -inf
        return False
    d = math.exp(f)
    if not (float(f32(d)) >= FLT_MIN) or not (d >= FLT_MIN):            # the result, or the value before rounding, is subnormal
        return False
    below = struct.unpack("<Q", struct.pack("<d", d))[0] & ((1 << 29) - 1)
    return abs(below - (1 << 28)) > (1 << 21)


def prec_groups(rec, off):
    out = []
    for g in range(len(off) - 1):
        out.append([pr.PRec(int(x["ref_id"]), int(x["start"]), int(x["end"]), int(x["aligned_len"]), int(x["query_aligned_len"]),
                            float(x["similarity"]), int(x["aln_score"]), bool(x["flags"] & _lib.REC_REVERSE))
                    for x in rec[int(off[g]):int(off[g + 1])]])
    return out


def restated(filters, txp_len, rec, off, rl, beta, source):
    """per kept alignment, in store order: (group, f) by the restatement"""
    F = fp.Filters(**filters)
    dt = fp.Store().dt
    out = []
    for g, (recs, n) in enumerate(zip(prec_groups(rec, off), rl)):
        if recs:
            out += [(g, a[4]) for a in pr.filter_projected(dt, F, txp_len, recs, int(n), beta, source)]
    return out


def tail_batch(txp_len, best, extra):
    """one group on transcript 0: the best record, one 0.1 below it and, with `extra`, a second best"""
    sims = [best, best - 0.1] + ([best] if extra else [])
    groups = [[pr.PRec(0, 1, int(txp_len[0]), 100, 100, s, 700) for s in sims]]
    return pr.pack(groups, [100])


# ---- 1: equals the one call -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("coverage", COVERAGES)
@pytest.mark.parametrize("source", pr.SOURCES)
def test_every_cutting_gives_the_one_calls_store(spr, source, coverage, monkeypatch):
    monkeypatch.setenv("OEM_KEEP_UNPACKED", "1")                        # (oem_debug_layout_hash reads the builders' streams)
    G = len(spr.group_off) - 1
    kw = dict(beta=spr.beta, prob_source=source)
    want_host = host_answer(spr.filters, spr.txp_len, spr.records, spr.group_off, spr.read_len, spr.beta, source)
    with _lib.testing() as L:
        long, want_kept, want_dt = DeviceStore.from_projected_records(spr.filters, spr.txp_len, spr.records, spr.group_off,
                                                                      spr.read_len, coverage=coverage, **kw)
        with long:
            assert long.n_reads == 3000 and np.array_equal(want_kept, spr.kept)
            want_hash = _hash(long) if coverage is None else None
            for name, sizes in cuttings(G).items():
                batches = synth.cut_projected_records(spr, sizes)
                assert [len(b[2]) for b in batches] == sizes
                with RecordsStream(spr.filters, spr.txp_len, coverage=coverage, projected=True, **kw) as s:
                    assert push_all(s, batches) == list(range(len(batches)))
                    one, kept, dt = s.finish()
                    info = s.info()
                with one:
                    same_store(one, long, coverage, (kept, dt), (want_kept, want_dt))
                    if coverage is None:
                        assert _hash(one) == want_hash, name
                assert info["batches"] == len(batches) and info["groups"] == G and info["records"] == len(spr.records)
                assert info["host_batches"] == 0
                assert info["host_finished"] == 0 or source != "score"   # (test 2 makes the host's share certain)
                with RecordsStream(spr.filters, spr.txp_len, coverage=coverage, projected=True, **kw) as s:   # the joined CSR itself
                    push_all(s, batches)
                    got, join_ms = finish_csr(L, s, coverage)
                csr_equals_host(got, want_host, want_kept, want_dt, coverage)


# ---- 2: the deferred expf is exercised --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unsure_input(spr):
    """the records with a hand-made tail of two batches, under beta 1000 and score_threshold 0: the tail's second records
    have f = -100, a subnormal result, which is never sure"""
    filters = dict(spr.filters, score_threshold=0.0)
    G = len(spr.group_off) - 1
    batches = synth.cut_projected_records(spr, [1] * 40 + [G - 40])
    batches += [tail_batch(spr.txp_len, 0.9, True), tail_batch(spr.txp_len, 0.8, False)]
    return filters, batches, concat(batches)


@pytest.mark.parametrize("source", pr.SOURCES)
def test_the_host_finishes_exactly_the_alignments_the_rule_leaves_unsure(spr, unsure_input, source):
    filters, batches, (rec, off, rl) = unsure_input
    beta = 1000.0
    assert len(batches) == 43
    alns = restated(filters, spr.txp_len, rec, off, rl, beta, source)
    unsure = [k for k, (_, f) in enumerate(alns) if not is_sure(f)]
    first_group = np.concatenate([[0], np.cumsum([len(b[2]) for b in batches])])
    batch_of = lambda k: int(np.searchsorted(first_group, alns[k][0], side="right") - 1)   # noqa: E731
    if source != "score":                                               # on the CPU first: the set is spread over batches
        tail = [k for k in unsure if batch_of(k) >= 41]
        assert len({batch_of(k) for k in unsure}) >= 2 and len(tail) == 2
        assert {k % 2 for k in tail} == {0, 1}                          # an odd and an even global alignment index
        assert all(float(alns[k][1]) == -100.0 or abs(float(alns[k][1]) + 100.0) < 1e-4 for k in tail)
    with RecordsStream(filters, spr.txp_len, projected=True, beta=beta, prob_source=source) as s:
        push_all(s, batches)
        one, kept, dt = s.finish()
        info = s.info()
    long, want_kept, want_dt = DeviceStore.from_projected_records(filters, spr.txp_len, rec, off, rl, beta=beta, prob_source=source)
    with one, long:
        assert one.nnz == len(alns)
        same_store(one, long, None, (kept, dt), (want_kept, want_dt))
    if source == "score":
        assert info["host_finished"] == 0
    else:
        assert info["host_finished"] == len(unsure) > 0
    with _lib.testing() as L, RecordsStream(filters, spr.txp_len, projected=True, beta=beta, prob_source=source) as s:
        push_all(s, batches)
        got, _ = finish_csr(L, s, None)
    csr_equals_host(got, host_answer(filters, spr.txp_len, rec, off, rl, beta, source), want_kept, want_dt, None)
    if source != "score":                                               # and by the restatement with libm's expf
        want_p = np.array([pr.libm_expf(f) for _, f in alns], dtype=np.float32)
        assert np.array_equal(got[2], want_p.view(np.uint32))


# ---- 3: the collect kernel's edges ------------------------------------------------------------------------------------
def test_the_collect_kernel_at_the_ballots_edges():
    """Batches whose lists have 0, 1, 63, 64 and 65 entries, and batches of 0, 2, 63, 64 and 65 alignments that are all
    unsure.  A group's best record has f = 0 and exp(0) = 1 is always sure, so a group of one kept record cannot be unsure:
    the first session has one unsure alignment per group of two (similarity, f = -100 behind the best), the second makes
    every alignment unsure under the combined source, where the best similarity and the best score sit on different
    records (f = -100 for either, -200 for a record that has neither)."""
    txp_len = np.full(5, 3000, dtype=np.uint64)
    filters = dict(five_prime_clip=2000, three_prime_clip=3000, score_threshold=0.0, min_aligned_fraction=0.5, min_aligned_len=50,
                   which_strand=1, score_prob_denom=5.0)
    rec_of = lambda t, sim, score: pr.PRec(t, 1, 3000, 100, 100, sim, score)   # noqa: E731
    two = lambda g: [rec_of(g % 5, 0.9, 700), rec_of((g + 1) % 5, 0.8, 700)]   # noqa: E731
    all2 = lambda g: [rec_of(g % 5, 0.9, 200), rec_of((g + 1) % 5, 0.8, 700)]   # noqa: E731
    all3 = lambda g: all2(g) + [rec_of((g + 2) % 5, 0.8, 200)]                  # noqa: E731

    def run(batches_of_groups, source, want_unsure):
        batches = [pr.pack(gs, [100] * len(gs)) for gs in batches_of_groups]
        rec, off, rl = concat(batches)
        alns = restated(filters, txp_len, rec, off, rl, 1000.0, source)
        assert sum(not is_sure(f) for _, f in alns) == sum(want_unsure)
        with _lib.testing() as L, RecordsStream(filters, txp_len, projected=True, beta=1000.0, prob_source=source) as s:
            push_all(s, batches)
            got, _ = finish_csr(L, s, None)
            info = s.info()
        assert info["host_finished"] == sum(want_unsure) and info["host_batches"] == 0
        want_p = np.array([pr.libm_expf(f) for _, f in alns], dtype=np.float32)
        assert len(got[1]) == len(alns) and np.array_equal(got[2], want_p.view(np.uint32))
        assert list(got[6]) == [len(g) for gs in batches_of_groups for g in gs]
        return got, want_p

    counts = [0, 1, 63, 64, 65]
    got, want_p = run([[two(g) for g in range(n)] for n in counts], "similarity", counts)
    assert len(want_p) == 2 * sum(counts) and np.all(want_p[0::2] == 1.0) and np.all(want_p[1::2] == pr.libm_expf(f32(-100.0)))
    assert 0.0 < float(want_p[1]) < FLT_MIN                            # subnormal: the host's expf, not the device's candidate
    kept_all = [[], [all2(0)], [all2(g) for g in range(30)] + [all3(30)], [all2(g) for g in range(32)],
                [all2(g) for g in range(31)] + [all3(31)]]
    sizes = [sum(len(g) for g in gs) for gs in kept_all]
    assert sizes == [0, 2, 63, 64, 65]
    got, want_p = run(kept_all, "combined", sizes)
    assert len(want_p) == sum(sizes) and np.all(want_p < FLT_MIN)      # host_finished == nnz: every alignment came from the host


# ---- 4: threads and tickets -------------------------------------------------------------------------------------------
def test_four_threads_push_and_the_tickets_give_the_order(spr):
    G = len(spr.group_off) - 1
    per = (G + 31) // 32
    batches = synth.cut_projected_records(spr, [per] * 31)
    assert len(batches) == 32
    tickets, errors = [None] * 32, []
    kw = dict(beta=1000.0, prob_source="similarity")                    # (as in test 2: every piece has a list to join)
    filters = dict(spr.filters, score_threshold=0.0)
    with RecordsStream(filters, spr.txp_len, coverage="logistic", projected=True, **kw) as s:
        def pusher(t):
            try:
                for k in range(t, 32, 4):
                    r, o, l = batches[k]
                    tickets[k] = s.push(r, o, read_len=l)
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
        assert s.info()["host_finished"] > 1000
    order = np.argsort(tickets)
    rec, off, rl = concat([batches[k] for k in order])
    long, want_kept, want_dt = DeviceStore.from_projected_records(filters, spr.txp_len, rec, off, rl, coverage="logistic", **kw)
    with one, long:
        same_store(one, long, "logistic", (kept, dt), (want_kept, want_dt))


# ---- 5: fallbacks -----------------------------------------------------------------------------------------------------
def test_a_big_score_sends_its_batch_and_an_infinite_beta_every_batch_through_the_host_loop(spr):
    G = len(spr.group_off) - 1
    batches = [tuple(a.copy() for a in b) for b in synth.cut_projected_records(spr, [G // 5] * 4)]
    assert len(batches) == 5
    batches[2][0]["aln_score"][len(batches[2][0]) // 2] = 2 ** 24 + 1
    rec, off, rl = concat(batches)
    with RecordsStream(spr.filters, spr.txp_len, projected=True, beta=spr.beta, prob_source="score") as s:
        push_all(s, batches)
        one, kept, dt = s.finish()
        info = s.info()
    assert info["host_batches"] == 1 and info["batches"] == 5 and info["host_finished"] == 0
    long, want_kept, want_dt = DeviceStore.from_projected_records(spr.filters, spr.txp_len, rec, off, rl, beta=spr.beta,
                                                                  prob_source="score")
    with one, long:
        same_store(one, long, None, (kept, dt), (want_kept, want_dt))
    inf = float("inf")                                                   # no device pass: the host loop's arrays, joined
    want = host_answer(spr.filters, spr.txp_len, rec, off, rl, inf, "similarity")
    with _lib.testing() as L, RecordsStream(spr.filters, spr.txp_len, coverage="logistic", projected=True, beta=inf) as s:
        push_all(s, batches)
        got, _ = finish_csr(L, s, "logistic")
        info = s.info()
    assert info["host_batches"] == 5 and info["host_finished"] == 0 and np.count_nonzero(want[1]) > 1000
    csr_equals_host(got, want, want[1], want[2], "logistic")


# ---- 6: the sticky error ----------------------------------------------------------------------------------------------
def test_a_bad_ref_id_is_sticky_and_names_ticket_record_and_ref_id(spr):
    G, T = len(spr.group_off) - 1, len(spr.txp_len)
    batches = synth.cut_projected_records(spr, [G // 5] * 4)
    n = max(len(b[0]) for b in batches)
    r2 = batches[2][0].copy()
    at = 41
    r2["ref_id"][at] = T
    r2["ref_id"][at + 100] = T + 5                                      # a later one: not the one named
    with RecordsStream(spr.filters, spr.txp_len, max_staged_records=n, projected=True, beta=spr.beta) as s:   # one batch at a time
        assert push_all(s, batches[:2]) + [s.push(r2, batches[2][1], read_len=batches[2][2])] == [0, 1, 2]
        for k in (3, 4):
            with pytest.raises(_lib.OemError) as ei:
                s.push(batches[k][0], batches[k][1], read_len=batches[k][2])
            assert ei.value.code == _lib.OEM_ERR_ARG
            msg = str(ei.value)
            assert "ticket 2:" in msg and f"record {at}:" in msg and f"ref_id {T} is not below n_txps" in msg
        h = C.c_void_p(1)
        assert s._lib.oem_records_stream_finish(s.handle, None, None, None, C.byref(h)) == _lib.OEM_ERR_ARG and not h.value
        assert b"ticket 2:" in s._lib.oem_last_error()
    tl = spr.txp_len.copy()
    zero = int(batches[2][0]["ref_id"][at])
    tl[zero] = 0
    first = int(np.flatnonzero(batches[2][0]["ref_id"] == zero)[0])
    with RecordsStream(spr.filters, tl, max_staged_records=n, projected=True, beta=spr.beta) as s:
        s.push(*batches[2][:2], read_len=batches[2][2])
        with pytest.raises(_lib.OemError) as ei:
            s.push(*batches[3][:2], read_len=batches[3][2])
        assert ei.value.code == _lib.OEM_ERR_ARG
        msg = str(ei.value)
        assert "ticket 0:" in msg and f"record {first}:" in msg and f"ref_id {zero} names a transcript of length 0" in msg


# ---- 7: empty and dropped-only sessions -------------------------------------------------------------------------------
@pytest.mark.parametrize("coverage", [None, "logistic"])
def test_sessions_without_a_kept_read_give_the_store_of_no_reads(spr, coverage):
    T = len(spr.txp_len)
    rev = lambda t: pr.PRec(t, 1, int(spr.txp_len[t]), 100, 100, 0.9, 500, reverse=True)   # noqa: E731  (which_strand is 1)
    dropped = pr.pack([[rev(0), rev(1)], [], [pr.PRec(2, 1, int(spr.txp_len[2]), 100, 100, 0.0, 500)]], [100, 100, 100])
    empty = (np.zeros(0, dtype=PROJ_RECORD), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint64))
    for batches in ([], [empty], [dropped], [empty, dropped, empty, dropped]):
        rec, off, rl = concat(batches)
        with RecordsStream(spr.filters, spr.txp_len, coverage=coverage, projected=True, beta=spr.beta) as s:
            push_all(s, batches)
            one, kept, dt = s.finish()
            info = s.info()
        long, want_kept, want_dt = DeviceStore.from_projected_records(spr.filters, spr.txp_len, rec, off, rl, beta=spr.beta,
                                                                      coverage=coverage)
        with one, long:
            assert (one.n_reads, one.nnz, one.n_txps) == (long.n_reads, long.nnz, long.n_txps) == (0, 0, T)
            assert np.array_equal(kept, want_kept) and len(kept) == len(off) - 1 and not kept.any() and dt == want_dt
        assert info["batches"] == len(batches) and info["host_finished"] == 0
        assert dt["discard_ori"] == 2 * sum(b is dropped for b in batches) and dt["valid_best_aln"] == 0


# ---- 8: the bulk drivers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True])
def test_the_genome_mode_bulk_drivers(spr, on_device, tmp_path):
    from oarfish_amd.bulk import (BulkArgs, perform_inference_and_write_output, quantify_genome_alignments_from_projected_batches,
                                  quantify_genome_alignments_from_projected_records)
    G, T = len(spr.group_off) - 1, len(spr.txp_len)
    txps = [f"ENST{i:011d}.{i % 13}" for i in range(T)]
    lens = [int(x) for x in spr.txp_len]
    names = [f"read{g}/{g % 7}" for g in range(G)]
    genomic = 1 + (np.arange(G) % 3 == 0).astype(np.int64)             # a third of the groups came from two genomic records
    kw = dict(beta=spr.beta, prob_source="similarity")
    mk = lambda out: BulkArgs(output=out, write_assignment_probs=True, display_thresh=1e-4, prob_on_device=on_device,   # noqa: E731
                              quant_on_device=on_device)
    out_b, out_r, out_h = (str(tmp_path / d / "sample") for d in ("batches", "records", "host"))

    batches, g0 = [], 0
    for r, o, l in synth.cut_projected_records(spr, [G // 3, G // 3]):
        batches.append((r, o, l, names[g0:g0 + len(l)], genomic[g0:g0 + len(l)]))
        g0 += len(l)
    assert len(batches) == 3 and g0 == G
    got_b, unique_b = quantify_genome_alignments_from_projected_batches(spr.filters, txps, lens, iter(batches), mk(out_b), **kw)
    got_r, unique_r = quantify_genome_alignments_from_projected_records(spr.filters, txps, lens, spr.records, spr.group_off,
                                                                        spr.read_len, mk(out_r), read_names=names,
                                                                        genomic_counts=genomic, **kw)
    want_unique = int(np.count_nonzero((spr.kept > 0) & (genomic == 1)))
    assert unique_b == unique_r == want_unique and 0 < want_unique < np.count_nonzero(spr.kept)

    # the host builder's store of the same groups, and perform_inference_and_write_output on it
    (row_ptr, tid, p, *_), kept, _ = host_answer(spr.filters, spr.txp_len, spr.records, spr.group_off, spr.read_len, spr.beta,
                                                 "similarity")
    rnames = [names[g] for g in np.flatnonzero(kept)]
    host = InMemoryAlignmentStore.from_arrays(row_ptr, tid, p)
    ref = perform_inference_and_write_output(host, txps, lens, BulkArgs(output=out_h, write_assignment_probs=True, display_thresh=1e-4),
                                             read_names=rnames)
    for got, what in ((got_b, "from batches"), (got_r, "from records")):
        assert_counts_close(got, ref, len(rnames), T, rtol=1e-10, what=f"the genome-mode driver {what} against the host store's")
    name_col = lambda path: [ln.split(b"\t")[0] for ln in open(path, "rb").read().split(b"\n")[T + 1:]]   # noqa: E731
    dev = host.device_store(T, 0)
    for out, got in ((out_b, got_b), (out_r, got_r)):
        # the same counts into both sides: the files byte for byte
        want_out = str(tmp_path / ("want_" + out.split("/")[-2]) / "sample")
        writers.write_output(want_out, {}, txps, lens, got, *dev.aux_counts())
        writers.write_out_prob(want_out, row_ptr, tid, dev.assignment_probs(got, 1e-4), rnames, txps, 1e-4)
        for ext in (".quant", ".ambig_info.tsv", ".prob"):
            assert open(out + ext, "rb").read() == open(want_out + ext, "rb").read(), (out, ext)
        assert name_col(out + ".prob") == name_col(out_h + ".prob") and len(name_col(out + ".prob")) == 3000 + 1
        assert open(out + ".ambig_info.tsv", "rb").read() == open(out_h + ".ambig_info.tsv", "rb").read()
        meta, meta_h = json.load(open(out + ".meta_info.json")), json.load(open(out_h + ".meta_info.json"))
        assert set(meta) == set(meta_h)
        for key in meta:                                                # field by field; the output path is each run's own
            assert meta[key] == (out if key == "output" else meta_h[key]), key
    if np.array_equal(got_b, got_r):
        for ext in (".quant", ".prob", ".ambig_info.tsv"):
            assert open(out_b + ext, "rb").read() == open(out_r + ext, "rb").read(), ext
    host.invalidate_device()
