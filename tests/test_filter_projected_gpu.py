"""GPU tests of the projected filter on the device (oem_filter_projected_device.hip):
oem_builder_add_projected_groups_device against the host batch byte for byte (random groups across chunk boundaries,
the edge list, the arguments on which a bare device exp would round the other way, the host-loop fallbacks, errors), and
oem_store_create_projected_records against the long way round for every coverage model and probability source."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from oarfish_amd import _lib, synth
from oarfish_amd.builder import PROJ_RECORD, StoreBuilder, filters_c
from oarfish_amd.types import DeviceStore
from oracle import filter_py as fp

from tests import projected_ref as pr
from tests.filter_common import filters_dict, state
from tests.projected_ref import last_projected_pass, libm_expf
from tests.test_filter_groups_gpu import _compare

pytestmark = pytest.mark.gpu

BETA = {"similarity": 10.0, "score": 10.0, "combined": 3.5}


# ---- device against host -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_batch():
    F, txp_len, groups, read_lens = pr.random_groups(31, 2000, T=120)
    F = dataclasses.replace(F, which_strand=0)                        # (the strand test has its edge groups; here rows are wanted)
    groups[1234] = [pr.PRec(j % 120, 5, int(txp_len[j % 120]), int(txp_len[j % 120]) - 4, 900, 0.97 - (j % 89) * 1e-3, 700 - j % 53,
                            reverse=j % 3 == 0) for j in range(300)]
    read_lens[1234] = 1000
    rec, off, rl = pr.pack(groups, read_lens)
    want = {}
    for source in pr.SOURCES:
        with StoreBuilder(filters_dict(F), txp_len) as b:
            kept = b.add_projected_groups(rec, off, rl, beta=BETA[source], prob_source=source)
            want[source] = (kept, state(b))
    return F, txp_len, groups, read_lens, rec, off, rl, want


@pytest.mark.parametrize("chunk", [1, 64, None])
@pytest.mark.parametrize("source", pr.SOURCES)
def test_device_batch_equals_the_host_batch(random_batch, source, chunk, monkeypatch):
    F, txp_len, _, _, rec, off, rl, want = random_batch
    want_kept, want_state = want[source]
    if chunk is not None:
        monkeypatch.setenv("OEM_FILTER_CHUNK_GROUPS", str(chunk))
    monkeypatch.setenv("OEM_FILTER_TIMING", "1")
    with _lib.testing() as L:
        with StoreBuilder(filters_dict(F), txp_len) as b:
            kept = b.add_projected_groups(rec, off, rl, beta=BETA[source], prob_source=source, device=0)
            got = state(b)
            measure_ms, emit_ms, _, n_host, nnz = last_projected_pass(L)
    assert measure_ms > 0 and emit_ms > 0 and nnz == int(want_kept.sum())   # the kernels ran: no silent host loop
    assert n_host == 0 if source == "score" else 0 < n_host < nnz           # the table / the candidate with its finish
    assert np.array_equal(kept, want_kept)
    assert got == want_state                                          # every exported array, the dims, the discard table
    assert want_kept.max() >= 100 and np.count_nonzero(want_kept) > 200 and (want_kept == 0).sum() > 200


def test_device_batch_appends_to_a_builder_that_holds_reads(random_batch):
    F, txp_len, groups, read_lens, rec, off, rl, _ = random_batch
    first = pr.pack(groups[:1500], read_lens[:1500])
    with StoreBuilder(filters_dict(F), txp_len) as h, StoreBuilder(filters_dict(F), txp_len) as d:
        assert h.add_projected_groups(*first).astype(bool).sum() >= 100 and d.add_projected_groups(*first).astype(bool).sum() >= 100
        kh = h.add_projected_groups(rec, off, rl, prob_source="combined")
        kd = d.add_projected_groups(rec, off, rl, prob_source="combined", device=0)
        assert np.array_equal(kh, kd) and state(h) == state(d)
        none = (np.zeros(0, dtype=PROJ_RECORD), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint64))
        assert d.add_projected_groups(*none, device=0).size == 0      # no groups
        assert state(h) == state(d)


# ---- edge groups -------------------------------------------------------------------------------------------------------
def _both(F, txp_len, groups, read_lens, beta, source):
    """the add_projected_group loop and the device batch on the same groups: (kept, export of the device's, its table)"""
    h, kh = pr.host_loop(F, txp_len, groups, read_lens, beta, source)
    with h, StoreBuilder(filters_dict(F), txp_len) as d:
        kd = d.add_projected_groups(*pr.pack(groups, read_lens), beta=beta, prob_source=source, device=0)
        assert np.array_equal(kh, kd), (kh, kd)
        assert state(h) == state(d)
        return kd, d.export(), d.discard_table()


@pytest.mark.parametrize("source", pr.SOURCES)
def test_edge_groups_one_by_one(source):
    seen = {}
    for name, F, txp_len, g, rl in pr.edge_groups():
        seen[name] = _both(F, txp_len, [g], [rl], 10.0, source)
    kept = {k: int(v[0][0]) for k, v in seen.items()}
    assert kept["empty"] == 0 and kept["one"] == 1 and seen["one"][1][2][0] == 1.0
    for name, counter in (("ori forward only", "discard_ori"), ("ori reverse only", "discard_ori"), ("aln_len", "discard_aln_len"),
                          ("3p", "discard_3p"), ("5p", "discard_5p"), ("score", "discard_score"), ("aln_frac", "discard_aln_frac")):
        dt = seen[name][2]
        assert dt[counter] == 1 and sum(dt.values()) - dt["valid_best_aln"] == 1, (name, dt)     # that reason alone
    assert kept["tie: the first decides the fraction"] == 0 and kept["tie: the first decides the fraction (kept)"] == 2
    for name in ("best similarity 0", "best similarity negative", "nan only"):
        assert kept[name] == 0 and sum(seen[name][2].values()) == 0                  # no counter moves
    assert kept["nan similarity"] == 1 and seen["nan similarity"][2]["discard_score"] == 2
    assert kept["read_len 0"] == 0 and kept["read_len 0, fraction 0 allowed"] == 1
    assert kept["threshold 1.5"] == 0 and seen["threshold 1.5"][2]["valid_best_aln"] == 1 and len(seen["threshold 1.5"][1][0]) == 1
    _, _, _, s, e, _ = seen["start 0 and end beyond the transcript"][1]
    assert list(s) == [1, 2000] and list(e) == [2000, 2000]                          # the clamps
    assert kept["score difference wraps"] == 2 and kept["huge similarities"] == 3     # the first through the host loop (2^24)
    if source != "score":
        assert list(seen["huge similarities"][1][2].view(np.uint32)) == [np.float32(1.0).view(np.uint32), 0, 0]   # expf(-inf)
    for n in (63, 64, 65, 300):
        assert kept[f"{n} records"] > n // 3


@pytest.mark.parametrize("n_groups", [130, 600])
def test_edge_groups_in_one_batch(n_groups):
    """the default-filter edge groups repeated: 130 groups cross a wavefront and a scan workgroup, 600 the kernels' too"""
    D = fp.Filters()
    pool = [(g, rl) for _, F, _, g, rl in pr.edge_groups() if F == D and all(abs(x.aln_score) <= 2 ** 24 for x in g)]
    picks = [pool[(7 * k) % len(pool)] for k in range(n_groups)]
    groups, read_lens = [p[0] for p in picks], [p[1] for p in picks]
    for source in pr.SOURCES:
        kept, (rp, tid, p, s, e, sd), dt = _both(D, [2000] * 8, groups, read_lens, 10.0, source)
        assert len(rp) - 1 == np.count_nonzero(kept) > n_groups // 3 and rp[-1] == kept.sum() == len(tid)
        assert dt["valid_best_aln"] + dt["discard_aln_frac"] <= sum(1 for g in groups if g)


# ---- the rounding case -------------------------------------------------------------------------------------------------
def _arguments_a_bare_exp_gets_wrong():
    """f32 in [-1, -2^-20] where float32(numpy.exp(float64(f))) differs from libm's expf(f), and as many where it does
    not.  libm is asked only where the f64 value lies within 1/64 ulp of a rounding tie: elsewhere its documented error
    before rounding (0.002 ulp) leaves it no choice."""
    bits = np.arange(np.float32(-2.0 ** -20).view(np.uint32), np.float32(-1.0).view(np.uint32), 41, dtype=np.uint32)
    f = bits.view(np.float32)
    assert len(f) > 3_000_000
    d = np.exp(f.astype(np.float64))
    below = (d.view(np.uint64) & np.uint64(2 ** 29 - 1)).astype(np.int64)
    near = np.flatnonzero(np.abs(below - 2 ** 28) <= 2 ** 23)
    naive = d.astype(np.float32)
    wrong = [int(i) for i in near if libm_expf(f[i]).view(np.uint32) != naive[i].view(np.uint32)]
    far = np.flatnonzero(np.abs(below - 2 ** 28) > 2 ** 26)[::50_000]
    return f, naive, wrong, [int(i) for i in far]


def test_arguments_where_a_bare_device_exp_would_round_the_other_way():
    f, naive, wrong, plain = _arguments_a_bare_exp_gets_wrong()
    assert len(wrong) >= 32 and len(plain) >= 32                      # about one in 12 000 differs
    F = fp.Filters(score_threshold=0.0)
    picks = wrong[:200] + plain[:64]
    groups, read_lens = [], []
    for k in range(0, len(picks), 3):                                 # best similarity exactly 1.0, beta 1: f comes out exactly
        groups.append([pr.PRec(0, 10, 1500, 1400, 1400, 1.0)] + [pr.PRec(1 + j, 10, 1500, 1400, 1400, 1.0 + float(f[i]))
                                                                 for j, i in enumerate(picks[k:k + 3])])
        read_lens.append(1500)
    rec, off, rl = pr.pack(groups, read_lens)
    txp_len = [2000] * 8
    for source in ("similarity", "combined"):
        with StoreBuilder(filters_dict(F), txp_len) as h:
            kh = h.add_projected_groups(rec, off, rl, beta=1.0, prob_source=source)
            want, p_host = state(h), h.export()[2]
        with _lib.testing() as L:
            with StoreBuilder(filters_dict(F), txp_len) as d:
                kd = d.add_projected_groups(rec, off, rl, beta=1.0, prob_source=source, device=0)
                got = state(d)
                _, _, _, n_host, nnz = last_projected_pass(L)
        assert np.array_equal(kh, kd) and int(kd.sum()) == nnz == len(picks) + len(groups)
        assert got == want                                            # bit for bit, the rounding cases included
        assert len(wrong[:200]) <= n_host < nnz                       # some finished by the host, some not
        # the case is real: the host's values are libm's, and the naive rounding differs on every picked argument
        got_p = np.concatenate([p_host[int(off[g]) + 1:int(off[g + 1])] for g in range(len(groups))])   # (every record is kept)
        n_w = len(wrong[:200])
        assert all(got_p[k].view(np.uint32) == libm_expf(f[i]).view(np.uint32) for k, i in enumerate(picks))
        assert all(got_p[k].view(np.uint32) != naive[i].view(np.uint32) for k, i in enumerate(picks[:n_w]))


# ---- fallbacks and errors ----------------------------------------------------------------------------------------------
def test_big_scores_a_bad_denominator_and_a_bad_beta_take_the_host_loop(random_batch, monkeypatch):
    F, txp_len, groups, read_lens, *_ = random_batch
    F = dataclasses.replace(F, which_strand=0, three_prime_clip=2 ** 62, five_prime_clip=2 ** 32 - 1)
    groups, read_lens = list(groups[:800]), list(read_lens[:800])
    monkeypatch.setenv("OEM_FILTER_TIMING", "1")
    with _lib.testing() as L:
        _both(F, txp_len, groups, read_lens, 10.0, "score")
        assert min(last_projected_pass(L)[:2]) > 0                                  # without the planted score: the device path
        groups[400] = [pr.PRec(3, 10, 250, 241, 900, 0.9, 2 ** 24 + 1), pr.PRec(4, 10, 250, 241, 900, 0.89, 2 ** 24 - 3)]
        read_lens[400] = 1000
        for source in pr.SOURCES:
            kept, (rp, tid, p, *_), _ = _both(F, txp_len, groups, read_lens, 10.0, source)
            measure_ms, emit_ms, *_ = last_projected_pass(L)
            assert measure_ms > 0 and emit_ms == 0                                  # found by the device pass, emitted by the host
            assert kept[400] == 2
        j = int(rp[np.count_nonzero(kept[:400])])
        assert p[j] == 1.0 and p[j + 1].view(np.uint32) != 0
        F0 = dataclasses.replace(F, score_prob_denom=0.0)
        kept, (rp, tid, p, *_), _ = _both(F0, txp_len, groups[:300], read_lens[:300], 10.0, "score")
        assert last_projected_pass(L)[:2] == (0.0, 0.0)                             # no table for D = 0: no device pass at all
        assert np.count_nonzero(kept) > 20 and np.all(np.isnan(p) | (p == 0))       # 0/0 and -g/0
        kept, (rp, tid, p, *_), _ = _both(F0, txp_len, groups[:300], read_lens[:300], 10.0, "combined")
        assert min(last_projected_pass(L)[:2]) > 0 and last_projected_pass(L)[3] > 0   # the device pass; the host finishes NaN and -inf
        for beta in (float("inf"), float("nan")):
            _both(F, txp_len, groups[:300], read_lens[:300], beta, "similarity")
            assert last_projected_pass(L)[:2] == (0.0, 0.0)                         # a beta that is not finite: the host loop


def test_argument_errors_in_a_middle_chunk(random_batch, monkeypatch):
    F, txp_len, groups, read_lens, *_ = random_batch
    groups, read_lens = list(groups[:300]), list(read_lens[:300])
    groups[150] = [pr.PRec(3, 10, 250, 241, 900, 0.9), pr.PRec(len(txp_len), 10, 250, 241, 900, 0.9)]
    groups[220] = [pr.PRec(len(txp_len) + 5, 10, 250, 241, 900, 0.9)]              # a later one: not the one named
    rec, off, rl = pr.pack(groups, read_lens)
    monkeypatch.setenv("OEM_FILTER_CHUNK_GROUPS", "100")
    with _lib.testing():
        with StoreBuilder(filters_dict(F), txp_len) as b:
            b.add_projected_groups(*pr.pack(groups[:50], read_lens[:50]))
            before = state(b)
            with pytest.raises(_lib.OemError) as ei:
                b.add_projected_groups(rec, off, rl, device=0)
            assert ei.value.code == _lib.OEM_ERR_ARG
            assert f"record {int(off[150]) + 1}:" in str(ei.value) and f"ref_id {len(txp_len)} " in str(ei.value)
            assert state(b) == before
            with pytest.raises(_lib.OemError) as ei:
                DeviceStore.from_projected_records(filters_dict(F), txp_len, rec, off, rl)
            assert ei.value.code == _lib.OEM_ERR_ARG and f"record {int(off[150]) + 1}:" in str(ei.value)
            bad = off.copy(); bad[9] = bad[10] + 1
            with pytest.raises(_lib.OemError) as ei:
                b.add_projected_groups(rec, bad, rl, device=0)
            assert ei.value.code == _lib.OEM_ERR_ARG and state(b) == before
        # a transcript of length 0, and *out is NULL on failure
        zero = np.array(txp_len, dtype=np.uint64); zero[7] = 0
        ok_rec, ok_off, ok_rl = pr.pack(groups[:150], read_lens[:150])
        first = int(np.flatnonzero(ok_rec["ref_id"] == 7)[0])
        fc = filters_c(filters_dict(F))
        po = _lib.ProjOptsC(10.0, 0)
        h = C.c_void_p(1)
        rc = _lib.lib().oem_store_create_projected_records(C.addressof(fc), zero.ctypes.data, len(zero), ok_rec.ctypes.data,
                                                           ok_off.ctypes.data, ok_rl.ctypes.data, 150, C.addressof(po), 100, -1,
                                                           2.0, 0, None, None, None, C.byref(h))
        msg = _lib.lib().oem_last_error().decode()
        assert rc == _lib.OEM_ERR_ARG and not h.value and f"record {first}:" in msg and "length 0" in msg


# ---- records -> store in one call ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recs():
    st = synth.make_store(5_000, 300, seed=511)
    sr = synth.make_projected_records(st, seed=512)
    names = [f"read{g}/{g % 7}" for g in range(len(sr.kept))]
    return sr, names


@pytest.fixture(scope="module")
def long_way(recs):
    sr, _ = recs
    builders = {}
    for source in pr.SOURCES:
        b = StoreBuilder(sr.filters, sr.txp_len)
        kept = b.add_projected_groups(sr.records, sr.group_off, sr.read_len, beta=sr.beta, prob_source=source)
        assert np.array_equal(kept, sr.kept) and b.discard_table() == sr.discard
        builders[source] = b
    yield builders
    for b in builders.values():
        b.close()


@pytest.mark.parametrize("source", pr.SOURCES)
@pytest.mark.parametrize("coding", [0, 2])
@pytest.mark.parametrize("coverage", [None, "logistic", "binomial"])
def test_one_call_store_equals_the_long_way_round(recs, long_way, coverage, coding, source):
    sr, names = recs
    b = long_way[source]
    one, got_kept, dt = DeviceStore.from_projected_records(sr.filters, sr.txp_len, sr.records, sr.group_off, sr.read_len,
                                                           beta=sr.beta, prob_source=source, coverage=coverage, weight_coding=coding)
    with one, b.device_store(coverage=coverage, weight_coding=coding) as long:
        assert np.array_equal(got_kept, sr.kept) and dt == b.discard_table()
        names_kept = [names[g] for g in np.flatnonzero(got_kept)]
        assert len(names_kept) == one.n_reads == 5_000
        counts = _compare(one, long, len(sr.txp_len), coverage, names_kept)
        assert abs(counts.sum() - one.n_reads) < 1e-6 * one.n_reads


def test_one_call_store_of_an_empty_input_and_of_dropped_reads_only():
    F = filters_dict(fp.Filters())
    tl = np.array([1000, 2000], dtype=np.uint64)
    none = (np.zeros(0, dtype=PROJ_RECORD), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint64))
    groups = [[pr.PRec(0, 1, 900, 900, 900, 0.0)], [], [pr.PRec(1, 1, 900, 900, 90, 0.9)]]    # best 0; empty; a tenth of the read
    for coverage in (None, "logistic"):
        for source in pr.SOURCES:
            st, kept, dt = DeviceStore.from_projected_records(F, tl, *none, prob_source=source, coverage=coverage)
            with st:
                assert (st.n_reads, st.nnz, st.n_txps) == (0, 0, 2) and len(kept) == 0 and sum(dt.values()) == 0
            st, kept, dt = DeviceStore.from_projected_records(F, tl, *pr.pack(groups, [900, 900, 900]), prob_source=source, coverage=coverage)
            with st:
                assert (st.n_reads, st.nnz) == (0, 0) and list(kept) == [0, 0, 0]
                assert dt["discard_aln_frac"] == 1 and sum(dt.values()) == 1
