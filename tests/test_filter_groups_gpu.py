"""GPU tests of the filter on the device (oem_filter_device.hip): oem_builder_add_groups_device against the host batch
byte for byte (random groups across chunk boundaries, the edge list, the host-loop fallbacks, errors), and
oem_store_create_records against the long way round (builder, add_groups, store from the builder) for every coverage
model, weight coding and layout builder."""
import ctypes as C

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth
from oarfish_amd.builder import ALN_RECORD, StoreBuilder
from oarfish_amd.types import DeviceStore
from oracle import filter_py as fp

from tests.common import assert_counts_close
from tests.filter_common import (edge_groups, filters_dict, host_loop, last_device_pass, libm_expf, pack, random_groups,
                                 state)

pytestmark = pytest.mark.gpu


# ---- device against host -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_batch():
    F, txp_len, groups = random_groups(31, 4000, T=120)
    rec, off = pack(groups)
    with StoreBuilder(filters_dict(F), txp_len) as b:
        kept = b.add_groups(rec, off)
        return F, txp_len, groups, rec, off, kept, state(b)


@pytest.mark.parametrize("chunk", [1, 64, 1000, None])
def test_device_batch_equals_the_host_batch(random_batch, chunk, monkeypatch):
    F, txp_len, groups, rec, off, want_kept, want = random_batch
    if chunk is not None:
        monkeypatch.setenv("OEM_FILTER_CHUNK_GROUPS", str(chunk))
    monkeypatch.setenv("OEM_FILTER_TIMING", "1")
    with _lib.testing() as L:
        with StoreBuilder(filters_dict(F), txp_len) as b:
            kept = b.add_groups(rec, off, device=0)
            got = state(b)
            measure_ms, emit_ms = last_device_pass(L)
    assert measure_ms > 0 and emit_ms > 0                             # the kernels ran: no silent host loop
    assert np.array_equal(kept, want_kept)
    assert got == want                                                # every exported array, the dims, the discard table
    assert want_kept.max() >= 2 and np.count_nonzero(want_kept) > 100 and (want_kept == 0).sum() > 100


def test_device_batch_appends_to_a_builder_that_holds_reads(random_batch):
    F, txp_len, groups, rec, off, _, _ = random_batch
    first = pack(groups[:3000])
    with StoreBuilder(filters_dict(F), txp_len) as h, StoreBuilder(filters_dict(F), txp_len) as d:
        assert h.add_groups(*first).astype(bool).sum() >= 100 and d.add_groups(*first).astype(bool).sum() >= 100
        kh = h.add_groups(rec, off)
        kd = d.add_groups(rec, off, device=0)
        assert np.array_equal(kh, kd) and state(h) == state(d)
        assert d.add_groups(np.zeros(0, dtype=ALN_RECORD), np.zeros(1, dtype=np.uint64), device=0).size == 0   # no groups
        assert state(h) == state(d)


# ---- edge groups -------------------------------------------------------------------------------------------------------
def _both(F, txp_len, groups):
    """the add_group loop and the device batch on the same groups: (host builder state, kept, export of the device's)"""
    h, kh = host_loop(F, txp_len, groups)
    with h, StoreBuilder(filters_dict(F), txp_len) as d:
        kd = d.add_groups(*pack(groups), device=0)
        assert np.array_equal(kh, kd), (kh, kd)
        assert state(h) == state(d)
        return kd, d.export(), d.discard_table()


def test_edge_groups_one_by_one():
    seen = {}
    for name, F, txp_len, g in edge_groups():
        seen[name] = _both(F, txp_len, [g])
    kept = {k: int(v[0][0]) for k, v in seen.items()}
    assert kept["empty"] == 0 and kept["one"] == 1 and kept["unmapped only"] == 0 and kept["non-positive best"] == 0
    assert seen["unmapped only"][2]["no_mapping"] == 1 and seen["non-positive best"][2]["no_valid_aln"] == 1
    for name, counter in (("ori forward only", "discard_ori"), ("ori reverse only", "discard_ori"), ("supp", "discard_supp"),
                          ("aln_len", "discard_aln_len"), ("3p", "discard_3p"), ("5p", "discard_5p"), ("score", "discard_score"),
                          ("aln_frac", "discard_aln_frac")):
        dt = seen[name][2]
        assert dt[counter] == 1 and sum(dt.values()) - dt["valid_best_aln"] == 1, (name, dt)     # that reason alone
    assert kept["tie: the first decides the fraction"] == 0 and kept["tie: the first decides the fraction (kept)"] == 2
    for name in ("no score, threshold 0", "no score, threshold -1"):                # kept with gap = best = 700
        p = seen[name][1][2]
        assert p[0] == 1.0 and p[1].view(np.uint32) == libm_expf(np.float32(-700.0) / np.float32(5.0)).view(np.uint32)
    assert kept["no score, threshold -1"] == 3 and kept["no score, default threshold"] == 1
    assert kept["seq_len on the third record"] == 3 and kept["no seq_len at all"] == 0
    assert kept["threshold 1.5"] == 0 and seen["threshold 1.5"][2]["valid_best_aln"] == 1 and len(seen["threshold 1.5"][1][0]) == 1
    p = seen["table end"][1][2]                                                     # gaps 0, 519, 520, 521, 1100 at D = 5
    assert kept["table end"] == 5 and p[0] == 1.0 and 0 < p[1] < 1.2e-38 and list(p[2:].view(np.uint32)) == [0, 0, 0]
    assert p[1].view(np.uint32) == libm_expf(np.float32(-519.0) / np.float32(5.0)).view(np.uint32)
    assert kept["clips at their defaults' extremes"] == 1 and kept["5p at u32 max"] == 1
    assert seen["5p at u32 max"][2]["discard_5p"] == 1
    for n in (63, 64, 65, 300):
        assert kept[f"{n} records"] > n // 3


@pytest.mark.parametrize("n_groups", [130, 600])
def test_edge_groups_in_one_batch(n_groups):
    """the default-filter edge groups repeated: 130 groups cross a wavefront and a scan workgroup, 600 the kernels' too"""
    D = fp.Filters()
    pool = [g for _, F, _, g in edge_groups() if F == D]
    groups = [pool[(7 * k) % len(pool)] for k in range(n_groups)]
    kept, (rp, tid, p, s, e, sd), dt = _both(D, [2000] * 8, groups)
    assert len(rp) - 1 == np.count_nonzero(kept) > n_groups // 3 and rp[-1] == kept.sum() == len(tid)
    assert dt["valid_best_aln"] + dt["no_mapping"] + dt["no_valid_aln"] + dt["discard_aln_frac"] == sum(1 for g in groups if g)


# ---- fallbacks and errors ----------------------------------------------------------------------------------------------
def test_scores_beyond_2_to_24_and_a_zero_denominator_take_the_host_loop(random_batch, monkeypatch):
    import dataclasses
    F, txp_len, groups, *_ = random_batch
    F = dataclasses.replace(F, which_strand=0, three_prime_clip=2 ** 62)            # (the two planted records pass the predicate)
    groups = list(groups[:1500])
    monkeypatch.setenv("OEM_FILTER_TIMING", "1")
    with _lib.testing() as L:
        _both(F, txp_len, groups)
        assert min(last_device_pass(L)) > 0                                         # without the planted score: the device path
        groups[700] = [fp.Rec(3, 10, 900, 800, 2 ** 24 + 1, 900), fp.Rec(4, 10, 900, 800, 2 ** 24 - 3, None)]
        kept, (rp, tid, p, *_), _ = _both(F, txp_len, groups)
        measure_ms, emit_ms = last_device_pass(L)
        assert measure_ms > 0 and emit_ms == 0                                      # found by the device pass, emitted by the host
        assert kept[700] == 2
        j = int(rp[np.count_nonzero(kept[:700])])
        want = np.exp(np.float32((np.float32(2 ** 24 - 3) - np.float32(2 ** 24 + 1)) / np.float32(F.score_prob_denom)))
        assert p[j] == 1.0 and abs(p[j + 1] - want) <= 2e-7 * want                  # f32(2^24 + 1) = 2^24: the gap is 3, not 4
        F0 = fp.Filters(score_prob_denom=0.0)
        kept, (rp, tid, p, *_), _ = _both(F0, txp_len, groups[:300])
        assert last_device_pass(L) == (0.0, 0.0)                                    # no table for D = 0: no device pass at all
        assert np.count_nonzero(kept) > 20 and np.all(np.isnan(p) | (p == 0))       # 0/0 and -g/0


def test_a_bad_ref_id_in_the_middle_chunk_is_an_argument_error(random_batch, monkeypatch):
    F, txp_len, groups, *_ = random_batch
    groups = list(groups[:300])
    groups[150] = [fp.Rec(3, 10, 900, 800, 500, 900), fp.Rec(len(txp_len), 10, 900, 800, 500, 900)]
    groups[220] = [fp.Rec(len(txp_len) + 5, 10, 900, 800, 500, 900)]                 # a later one: not the one named
    rec, off = pack(groups)
    monkeypatch.setenv("OEM_FILTER_CHUNK_GROUPS", "100")
    with _lib.testing():
        with StoreBuilder(filters_dict(F), txp_len) as b:
            b.add_groups(*pack(groups[:50]))
            before = state(b)
            with pytest.raises(_lib.OemError) as ei:
                b.add_groups(rec, off, device=0)
            assert ei.value.code == _lib.OEM_ERR_ARG
            assert f"record {int(off[150]) + 1}:" in str(ei.value) and f"ref_id {len(txp_len)} " in str(ei.value)
            assert state(b) == before
            with pytest.raises(_lib.OemError) as ei:
                DeviceStore.from_records(filters_dict(F), txp_len, rec, off)
            assert ei.value.code == _lib.OEM_ERR_ARG and f"record {int(off[150]) + 1}:" in str(ei.value)
            bad = off.copy(); bad[9] = bad[10] + 1
            with pytest.raises(_lib.OemError) as ei:
                b.add_groups(rec, bad, device=0)
            assert ei.value.code == _lib.OEM_ERR_ARG and state(b) == before


# ---- records -> store in one call ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recs():
    st = synth.make_store(20_000, 500, seed=411)
    sr = synth.make_records(st, seed=412)
    b = StoreBuilder(sr.filters, sr.txp_len)
    kept = b.add_groups(sr.records, sr.group_off)
    assert np.array_equal(kept, sr.kept) and b.discard_table() == sr.discard
    names = [f"read{g}/{g % 7}" for g in range(len(kept))]
    yield sr, b, kept, names
    b.close()


def _compare(one, long, T, coverage, names_kept):
    assert (one.n_reads, one.nnz, one.n_txps) == (long.n_reads, long.nnz, long.n_txps)
    for a, b in zip(one.aux_counts(), long.aux_counts()):
        assert np.array_equal(a, b)
    ca, ia = one.em_run()
    cb, ib = long.em_run()
    assert ia.niter == ib.niter
    if coverage is None:       # bit-identical weights: the same-iteration tolerance, rtol 1e-10 over the floor of DESIGN section 2
        assert_counts_close(ca, cb, one.n_reads, T, rtol=1e-10, what="records -> store")
    else:                      # two coverage passes, f64 atomic order: as test_store_coverage_gpu.py holds the one-call store
        np.testing.assert_allclose(ca, cb, rtol=1e-10, atol=1e-10)
    ta = one.assignment_text(cb, 1e-3, read_names=names_kept)     # the same counts into both: the same bytes out
    tb = long.assignment_text(cb, 1e-3, read_names=names_kept)
    assert ta.text.tobytes() == tb.text.tobytes() and np.array_equal(ta.kept, tb.kept)
    return ca


@pytest.mark.parametrize("layout_build", [0, 1])
@pytest.mark.parametrize("coding", [0, 1, 2])
@pytest.mark.parametrize("coverage", [None, "logistic", "binomial"])
def test_one_call_store_equals_the_long_way_round(recs, coverage, coding, layout_build):
    sr, b, kept, names = recs
    T = len(sr.txp_len)
    kw = dict(weight_coding=coding, layout_build=layout_build)
    one, got_kept, dt = DeviceStore.from_records(sr.filters, sr.txp_len, sr.records, sr.group_off, coverage=coverage, **kw)
    with one, b.device_store(coverage=coverage, **kw) as long:
        assert np.array_equal(got_kept, kept) and dt == b.discard_table()
        names_kept = [names[g] for g in np.flatnonzero(got_kept)]
        assert len(names_kept) == one.n_reads == 20_000
        counts = _compare(one, long, T, coverage, names_kept)
        assert abs(counts.sum() - one.n_reads) < 1e-6 * one.n_reads


@pytest.mark.parametrize("coverage", [None, "logistic"])
def test_one_call_store_when_the_host_layout_builder_takes_it(recs, coverage, monkeypatch):
    """the device tiler declines (forced): row pointers and ids come back from the device for the host builder"""
    sr, b, kept, names = recs
    monkeypatch.setenv("OEM_TEST_HOST_LAYOUT", "1")
    monkeypatch.setenv("OEM_KEEP_UNPACKED", "1")                      # (oem_debug_layout_hash reads the builders' streams)
    monkeypatch.setenv("OEM_FILTER_CHUNK_GROUPS", "3000")
    monkeypatch.setenv("OEM_FILTER_TIMING", "1")
    with _lib.testing() as L:
        one, got_kept, dt = DeviceStore.from_records(sr.filters, sr.txp_len, sr.records, sr.group_off, coverage=coverage)
        assert min(last_device_pass(L)) > 0                            # the records were filtered by the kernels
        with one:
            out = (C.c_uint64 * 18)()
            one._check(one._lib.oem_debug_layout_hash(one.handle, out, 15))
            assert out[14] == 0                                       # the host built the layout
            ca, ia = one.em_run()
    with b.device_store(coverage=coverage) as long:
        cb, ib = long.em_run()
    assert np.array_equal(got_kept, kept) and dt == b.discard_table() and ia.niter == ib.niter
    np.testing.assert_allclose(ca, cb, rtol=1e-10, atol=1e-10)


def test_one_call_store_of_an_empty_input_and_of_dropped_reads_only():
    F = filters_dict(fp.Filters())
    tl = np.array([1000, 2000], dtype=np.uint64)
    for coverage in (None, "logistic"):
        st, kept, dt = DeviceStore.from_records(F, tl, np.zeros(0, dtype=ALN_RECORD), np.zeros(1, dtype=np.uint64), coverage=coverage)
        with st:
            assert (st.n_reads, st.nnz, st.n_txps) == (0, 0, 2) and len(kept) == 0 and sum(dt.values()) == 0
        groups = [[fp.Rec(0, 0, 0, 0, None, 100, unmapped=True)], [], [fp.Rec(1, 10, 900, 800, 0, 900)]]
        st, kept, dt = DeviceStore.from_records(F, tl, *pack(groups), coverage=coverage)
        with st:
            assert (st.n_reads, st.nnz) == (0, 0) and list(kept) == [0, 0, 0] and dt["no_mapping"] == dt["no_valid_aln"] == 1


def test_one_call_store_errors():
    F = filters_dict(fp.Filters())
    tl = np.array([1000, 2000], dtype=np.uint64)
    rec, off = pack([[fp.Rec(0, 10, 900, 890, 500, 900)], [fp.Rec(1, 10, 2600, 2590, 500, 2600)]])   # past transcript 1's end
    with pytest.raises(oarfish_amd.OemError) as ei:
        DeviceStore.from_records(F, tl, rec, off, coverage="logistic")
    assert ei.value.code == _lib.OEM_ERR_STATE and "outside its transcript" in str(ei.value)
    st, kept, _ = DeviceStore.from_records(F, tl, rec, off)           # without a coverage model the store exists
    with st:
        assert list(kept) == [1, 1] and st.n_reads == 2
    L = _lib.lib()
    fc = oarfish_amd.builder.filters_c(F)
    h = C.c_void_p(1)
    args = lambda model, bw, o: (C.addressof(fc), tl.ctypes.data, 2, rec.ctypes.data, off.ctypes.data, 2, bw, model, 2.0, 0,  # noqa: E731
                                 o, None, None, C.byref(h))
    assert L.oem_store_create_records(*args(2, 100, None)) == _lib.OEM_ERR_ARG and not h.value
    assert L.oem_store_create_records(*args(0, 0, None)) == _lib.OEM_ERR_ARG
    o = _lib.StoreOptsC(); o.weight_coding = 3
    assert L.oem_store_create_records(*args(-1, 100, C.addressof(o))) == _lib.OEM_ERR_ARG
