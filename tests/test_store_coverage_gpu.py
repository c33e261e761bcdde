"""GPU tests of the bulk coverage model + store creation in one call (oem_store_create_coverage /
DeviceStore.with_coverage): the store equals oem_coverage_probs_device followed by oem_store_create on that column --
layout hashes on every layout path and weight coding, the caller-order store, the returned column, the oracle under
both gates, the steps after the EM, f32 rounding edge cases, the builder variant, errors, the bulk driver and the
full BASELINE configs[2] size.
The whole-store kernels at bin, length and span edges: test_coverage_edges_gpu.py (grid: coverage_edges_common.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, bulk, synth
from oarfish_amd.types import DeviceStore, InMemoryAlignmentStore
from oracle import c_oracle
from oracle import filter_py as fp

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 4)
MODELS = {"logistic": 0, "binomial": 1}


def _cov_device(rp, tid, s, e, tl, model="logistic", growth=2.0, bin_width=100):
    out = np.empty(len(tid))
    _lib.check(_lib.lib().oem_coverage_probs_device(rp.ctypes.data, tid.ctypes.data, s.ctypes.data, e.ctypes.data,
                                                    tl.ctypes.data, len(rp) - 1, len(tid), len(tl), bin_width,
                                                    MODELS[model], growth, 0, out.ctypes.data))
    return out


def _hash(store):
    out = (C.c_uint64 * 18)()
    store._check(store._lib.oem_debug_layout_hash(store.handle, out, 18))
    return list(out)


@pytest.fixture(scope="module")
def medium():
    """~200 k reads over 20 k transcripts, a few zero-span alignments."""
    st = synth.make_store(200_000, 20_000, seed=311, threads=THREADS)
    tl, s, e = synth.make_coordinates(st.tid, st.n_txps, seed=311, zero_span_frac=0.002, threads=THREADS)
    return st.row_ptr, st.tid, st.as_prob, s, e, tl


# ---- bit-identical layouts -----------------------------------------------------------------------------------------
PATHS = ["default", "reorder_2", "layout_build_1", "host_layout", "weights_pass"]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("coding", [0, 1, 2])
@pytest.mark.parametrize("model", ["logistic", "binomial"])
def test_layout_equals_the_composition(medium, model, coding, path, monkeypatch):
    rp, tid, p, s, e, tl = medium
    monkeypatch.setenv("OEM_KEEP_UNPACKED", "1")
    kw = dict(weight_coding=coding)
    if path == "reorder_2":
        kw["reorder_rows"] = 2
    elif path == "layout_build_1":
        kw["layout_build"] = 1
    elif path == "host_layout":     # the device builder declines: the weights come back from the device
        monkeypatch.setenv("OEM_TEST_HOST_LAYOUT", "1")
    elif path == "weights_pass":    # the weights in a pass of their own instead of k_cov_reads' epilogue
        monkeypatch.setenv("OEM_COV_WEIGHTS_PASS", "1")
    with _lib.testing():
        fused, cov = DeviceStore.with_coverage(rp, tid, p, s, e, tl, model=model, return_coverage=True, **kw)
        with fused:
            got = _hash(fused)
            n_dict = fused.info(_lib.OEM_INFO_WEIGHT_DICT_ENTRIES)
            with DeviceStore(rp, tid, p, cov, len(tl), **kw) as comp:
                want = _hash(comp)
                assert n_dict == comp.info(_lib.OEM_INFO_WEIGHT_DICT_ENTRIES) == 0
    assert np.isnan(cov).sum() > 0
    assert got == want, (model, coding, path)
    if path in ("layout_build_1", "host_layout"):
        assert got[14] == 0
    else:
        assert got[14] == 1


def test_caller_order_store_agrees(medium):
    """reorder_rows = 1: no tiled layout; m_step and em_run on the fused store agree with the composition's."""
    rp, tid, p, s, e, tl = medium
    T = len(tl)
    theta = np.random.default_rng(5).random(T) + 0.1
    for coding in (0, 2):
        with DeviceStore.with_coverage(rp, tid, p, s, e, tl, reorder_rows=1, weight_coding=coding,
                                       return_coverage=True)[0] as fused:
            cov = _cov_device(rp, tid, s, e, tl)
            with DeviceStore(rp, tid, p, cov, T, reorder_rows=1, weight_coding=coding) as comp:
                np.testing.assert_allclose(fused.m_step(theta), comp.m_step(theta), rtol=1e-12, atol=0)
                a, ia = fused.em_run(max_iter=300)
                b, ib = comp.em_run(max_iter=300)
                assert ia.niter == ib.niter
                np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("model", ["logistic", "binomial"])
def test_returned_column_is_the_coverage_call(medium, model):
    rp, tid, p, s, e, tl = medium
    st, cov = DeviceStore.with_coverage(rp, tid, p, s, e, tl, model=model, growth_rate=0.8, return_coverage=True)
    st.close()
    want = _cov_device(rp, tid, s, e, tl, model, 0.8)
    assert np.isnan(want).sum() > 0
    assert np.array_equal(np.isnan(cov), np.isnan(want))
    fin = ~np.isnan(want)
    np.testing.assert_allclose(cov[fin], want[fin], rtol=1e-12, atol=0)


# ---- the oracle, and the steps after the EM --------------------------------------------------------------------------
@pytest.mark.parametrize("gate", [50, 1])
def test_em_matches_the_oracle(gate):
    T = 400
    st = synth.make_store(3_000, T, seed=53)
    tl, s, e = synth.make_coordinates(st.tid, T, seed=53, zero_span_frac=0.005)
    fst = fp.Store(row_ptr=[int(x) for x in st.row_ptr], tid=[int(x) for x in st.tid], start=[int(x) for x in s],
                   end=[int(x) for x in e])
    want_cov = np.asarray(fp.coverage_probs(fst, [int(x) for x in tl], 100, 2.0, model="logistic"))
    assert np.isnan(want_cov).sum() > 0
    o = c_oracle.Store(st.row_ptr, st.tid, st.as_prob, want_cov, T)
    want, wi = c_oracle.do_em(o, max_iter=1000, conv_thresh=1e-3, min_iter_gate=gate)
    for coding in (0, 1):
        with DeviceStore.with_coverage(st.row_ptr, st.tid, st.as_prob, s, e, tl, weight_coding=coding) as d:
            got, gi = d.em_run(max_iter=1000, conv_thresh=1e-3, min_iter_gate=gate)
        assert gi.niter == wi.niter, (gate, coding)
        np.testing.assert_allclose(got, want, rtol=1e-8, atol=1e-9)


def test_bootstrap_aux_counts_and_assignment_probs_agree(medium):
    rp, tid, p, s, e, tl = medium
    T = len(tl)
    fused, cov = DeviceStore.with_coverage(rp, tid, p, s, e, tl, return_coverage=True)
    with fused, DeviceStore(rp, tid, p, cov, T) as comp:
        bf, inf_f = fused.bootstrap(3, seed=11, max_iter=200)
        bc, inf_c = comp.bootstrap(3, seed=11, max_iter=200)
        assert [i.niter for i in inf_f] == [i.niter for i in inf_c]
        np.testing.assert_allclose(bf, bc, rtol=1e-10, atol=1e-10)
        for x, y in zip(fused.aux_counts(), comp.aux_counts()):
            np.testing.assert_array_equal(x, y)
        counts, _ = comp.em_run(max_iter=200)
        np.testing.assert_allclose(fused.assignment_probs(counts, 1e-6), comp.assignment_probs(counts, 1e-6),
                                   rtol=1e-12, atol=1e-15)


def test_f32_rounding_edge_cases(monkeypatch):
    """Products p * cov that land in f32 subnormals and below FLT_TRUE_MIN: the coding-2 store is the one
    oem_store_create builds from the returned column (the host's (float) cast)."""
    T = 300
    st = synth.make_store(20_000, T, seed=71)
    tl, s, e = synth.make_coordinates(st.tid, T, seed=71, zero_span_frac=0.002)
    tiny = np.array([1e-30, 1e-37, 1e-38, 3e-39, 1e-40, 1e-43, 4e-45, 1.4e-45, 0.0], dtype=np.float32)
    p = st.as_prob.copy()
    p[::3] = tiny[np.arange(len(p[::3])) % len(tiny)]
    monkeypatch.setenv("OEM_KEEP_UNPACKED", "1")
    with _lib.testing():
        fused, cov = DeviceStore.with_coverage(st.row_ptr, st.tid, p, s, e, tl, weight_coding=2, return_coverage=True)
        prod = (p.astype(np.float64) * np.nan_to_num(cov, nan=0.0)).astype(np.float32)
        assert np.any((prod > 0) & (prod < np.finfo(np.float32).tiny))   # subnormal products occur
        assert np.any((p > 0) & (cov > 0) & (prod == 0))                  # and products that round to 0
        with fused, DeviceStore(st.row_ptr, st.tid, p, cov, T, weight_coding=2) as comp:
            assert _hash(fused) == _hash(comp)


def test_builder_variant():
    T = 200
    txp_len = np.random.default_rng(3).integers(500, 3000, size=T).astype(np.uint64)
    F = fp.Filters()
    F.min_aligned_len, F.min_aligned_fraction, F.score_threshold = 0, 0.0, 0.0
    fc = _lib.FiltersC(F.five_prime_clip, F.three_prime_clip, F.score_threshold, F.min_aligned_fraction,
                       F.min_aligned_len, F.which_strand, F.score_prob_denom, 0)
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.oem_builder_create(C.addressof(fc), txp_len.ctypes.data, T, C.byref(h)))
    try:
        rng = np.random.default_rng(4)
        recs = (_lib.AlnRecordC * 8)()
        kept = C.c_uint32(0)
        for _ in range(3_000):
            k = int(rng.integers(1, 6))
            for q in range(k):
                t = int(rng.integers(0, T))
                span = int(min(rng.integers(100, 1500), txp_len[t]))
                a = int(rng.integers(0, int(txp_len[t]) - span + 1))
                recs[q] = _lib.AlnRecordC(t, a, a + span, span, 1000 - 7 * q, span, _lib.REC_HAS_SCORE, 0)
            _lib.check(L.oem_builder_add_group(h, recs, k, C.byref(kept)))
        R, nnz = C.c_uint64(0), C.c_uint64(0)
        _lib.check(L.oem_builder_dims(h, C.byref(R), C.byref(nnz)))
        for coding in (0, 2):
            o = _lib.StoreOptsC()
            o.weight_coding = coding
            col = np.empty(nnz.value)
            fs = C.c_void_p()
            _lib.check(L.oem_builder_store_create_coverage(h, 100, 0, 2.0, 0, C.addressof(o), col.ctypes.data,
                                                           C.byref(fs)))
            want = np.empty(nnz.value)
            _lib.check(L.oem_builder_coverage_probs_device(h, 100, 0, 2.0, 0, want.ctypes.data))
            np.testing.assert_allclose(col, want, rtol=1e-12, atol=0)
            cs = C.c_void_p()
            _lib.check(L.oem_builder_store_create(h, col.ctypes.data, 0, C.addressof(o), C.byref(cs)))
            try:
                outs = []
                for handle in (fs, cs):
                    c = np.zeros(T)
                    ri = _lib.RunInfoC()
                    _lib.check(L.oem_em_run(handle, None, 500, 1e-3, 50, c.ctypes.data, C.byref(ri)))
                    outs.append((c, ri.niter))
                assert outs[0][1] == outs[1][1]
                np.testing.assert_allclose(outs[0][0], outs[1][0], rtol=1e-12, atol=1e-12)
            finally:
                L.oem_store_destroy(fs)
                L.oem_store_destroy(cs)
    finally:
        L.oem_builder_destroy(h)


# ---- empty and faulty stores -----------------------------------------------------------------------------------------
def test_empty_store():
    tl = np.array([1000, 2000], dtype=np.uint64)
    z32 = np.zeros(0, np.uint32)
    for rp in (np.zeros(1, np.uint64), np.zeros(4, np.uint64)):   # no reads; reads without alignments
        for coding in (0, 2):
            with DeviceStore.with_coverage(rp, z32, np.zeros(0, np.float32), z32, z32, tl, weight_coding=coding,
                                           return_coverage=True)[0] as d:
                assert (d.n_reads, d.nnz, d.n_txps) == (len(rp) - 1, 0, 2)
                with DeviceStore(rp, z32, np.zeros(0, np.float32), np.zeros(0), 2, weight_coding=coding) as c:
                    a, ia = d.em_run(max_iter=10)
                    b, ib = c.em_run(max_iter=10)
                    assert ia.niter == ib.niter
                    np.testing.assert_array_equal(a, b)


def test_an_alignment_past_its_transcript():
    T = 300
    st = synth.make_store(5_000, T, seed=89)
    tl, s, e = synth.make_coordinates(st.tid, T, seed=89)
    e_bad = e.copy()
    j = len(e) // 2
    e_bad[j] = np.uint32(int(tl[st.tid[j]]) + 500)
    with pytest.raises(oarfish_amd.OemError) as want:
        _cov_device(st.row_ptr, st.tid, s, e_bad, tl)
    with pytest.raises(oarfish_amd.OemError) as got:
        DeviceStore.with_coverage(st.row_ptr, st.tid, st.as_prob, s, e_bad, tl)
    assert got.value.code == want.value.code == _lib.OEM_ERR_STATE
    assert str(got.value) == str(want.value) and "outside its transcript" in str(got.value)
    with DeviceStore.with_coverage(st.row_ptr, st.tid, st.as_prob, s, e, tl) as d:   # the device is still usable
        d.em_run(max_iter=10)


# ---- the bulk driver -------------------------------------------------------------------------------------------------
def _read_quant(path):
    with open(path + ".quant") as f:
        next(f)
        return np.array([float(line.split("\t")[2]) for line in f])


def test_bulk_driver_with_coverage(tmp_path):
    T = 2_000
    st = synth.make_store(40_000, T, seed=97)
    tl, s, e = synth.make_coordinates(st.tid, T, seed=97, zero_span_frac=0.001)
    names = [f"t{i}" for i in range(T)]
    fused = InMemoryAlignmentStore.from_arrays(st.row_ptr, st.tid, st.as_prob)
    out_f = str(tmp_path / "fused")
    cf = bulk.perform_inference_and_write_output(fused, names, tl, bulk.BulkArgs(output=out_f),
                                                 coverage=bulk.BulkCoverage(s, e))
    assert fused.filter_opts.model_coverage
    cov = _cov_device(st.row_ptr, st.tid, s, e, tl)
    assert np.array_equal(np.isnan(fused.coverage_probabilities), np.isnan(cov))
    comp = InMemoryAlignmentStore.from_arrays(st.row_ptr, st.tid, st.as_prob, cov, model_coverage=True)
    out_c = str(tmp_path / "comp")
    cc = bulk.perform_inference_and_write_output(comp, names, tl, bulk.BulkArgs(output=out_c))
    np.testing.assert_allclose(cf, cc, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(_read_quant(out_f), _read_quant(out_c), rtol=1e-10, atol=1e-10)
    with open(out_f + ".meta_info.json") as f:
        assert json.load(f)["filter_options"]["model_coverage"] is True
    # the driver used the resident store the coverage step installed: no second one was made
    assert len(fused._dev) == 1 and list(fused._dev.values())[0][0][3] is fused.coverage_probabilities
    plain = InMemoryAlignmentStore.from_arrays(st.row_ptr, st.tid, st.as_prob)
    c0 = bulk.perform_inference_and_write_output(plain, names, tl, bulk.BulkArgs(output=str(tmp_path / "plain")))
    assert not plain.filter_opts.model_coverage and not np.allclose(c0, cf)


# ---- full size -------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(1200)
def test_full_c3_size():
    """BASELINE configs[2] shape (10 M reads, 200 k transcripts): the fused call against the composition."""
    st = synth.make_store(10_000_000, 200_000, threads=THREADS)
    tl, s, e = synth.make_coordinates(st.tid, st.n_txps, threads=THREADS)
    with DeviceStore.with_coverage(st.row_ptr, st.tid, st.as_prob, s, e, tl) as d:
        a, ia = d.em_run()
    cov = _cov_device(st.row_ptr, st.tid, s, e, tl)
    with DeviceStore(st.row_ptr, st.tid, st.as_prob, cov, st.n_txps) as d:
        b, ib = d.em_run()
    assert ia.niter == ib.niter
    np.testing.assert_allclose(a, b, rtol=1e-10, atol=1e-10)
