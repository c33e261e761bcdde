"""The per-iteration rel_diff record on the device (OEM_OPT_RUN_HISTORY, oem_run_history): every loop driver's
record against the trajectory of the oracle's single pass with em.rs:194-218 applied in NumPy
(tests/run_history_common.py), which is itself held to c_oracle.do_em's / em_par's iteration count and convergence
flag.  Per entry the tolerance is the one tests/test_gpu_parity.py holds info.rel_diff to; the last entry is
info.rel_diff bit for bit; the length is niter + converged = n_passes - 1."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import threading

import numpy as np
import pytest

from oarfish_amd import _lib, dist as odist, synth
from oarfish_amd.types import DeviceStore
from oracle import c_oracle, resample_np
from tests.common import assert_counts_close
from tests.run_history_common import check_history, close, oracle_history

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, R, T = 4711, 60_000, 3_000


def _store(coverage=False):
    return synth.make_store(R, T, seed=SEED, coverage=coverage)


def _init():
    return np.random.default_rng(3).lognormal(0, 1.0, T) * R / T


# (max_iter, thresh, gate, init?): two runs that converge, two that reach max_iter (the deferred loop decides their last
# iteration by the sweep), both gates, with and without init_abundances
CASES = [(1000, 1e-3, 50, False), (1000, 1e-3, 1, False), (1000, 1e-2, 1, True), (60, 0.0, 50, False), (45, 0.0, 1, True),
         (300, 1e-3, 50, True)]


def _run_and_check(d, o, n_reads, max_iter, thresh, gate, init, what, em_par=False):
    d.set_option(_lib.OEM_OPT_RUN_HISTORY, max_iter)
    cnt, info = d.em_run(init, max_iter, thresh, gate)
    want = oracle_history(o, n_reads, init, max_iter, thresh, gate)
    if em_par:
        _, wi = c_oracle.em_par(o, init=init, max_iter=max_iter, conv_thresh=thresh, min_iter_gate=gate)
    else:
        _, wi = c_oracle.do_em(o, init=init, max_iter=max_iter, conv_thresh=thresh, min_iter_gate=gate)
    assert (want[1], want[2]) == (wi.niter, wi.converged), (what, want[1:], wi)   # the test's own loop, held to the oracle
    check_history(d.run_history(0), d.run_history_len(0), info, want, what)
    return cnt, info


def _cases_on(d, o, st, what, cases=CASES):
    for m, th, g, with_init in cases:
        _run_and_check(d, o, st.n_reads, m, th, g, _init() if with_init else None,
                       f"{what}: max_iter {m}, thresh {th}, gate {g}, init {with_init}", em_par=(g == 1))


def test_deferred_loop_records_every_iteration():
    """run_em_deferred: deferred_decide reached from the fold launch and, for the runs that end at max_iter, from
    k_deferred_sweep."""
    st = _store()
    o = c_oracle.Store(st.row_ptr, st.tid, st.as_prob, None, T)
    with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, T) as d:
        assert d.info(_lib.OEM_INFO_TILES) > 0
        _cases_on(d, o, st, "deferred")


def test_deferred_loop_without_remote_alignments_records_through_the_decide_kernel():
    """a store without remote alignments has no fold launch: k_deferred_decide applies the rule"""
    st = synth.make_store(R, T, seed=SEED + 1, far="paralog_adjacent")
    o = c_oracle.Store(st.row_ptr, st.tid, st.as_prob, None, T)
    with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, T) as d:
        assert d.info(_lib.OEM_INFO_REMOTE_ALIGNMENTS) == 0
        _cases_on(d, o, st, "deferred, no remote", CASES[:1] + CASES[3:4])


@pytest.mark.parametrize("how", ["deferred_off", "caller_order", "graph"])
def test_classic_loop_records_every_iteration(how, monkeypatch):
    """k_reldiff_swap_clear: the tiled store with the deferred rule switched off (test-only library), the caller-order
    CSR (reorder_rows = 1), and the captured-graph replay of run_em_device -- OEM_GRAPH=1 in the test-only library makes
    graph_ok hold, and every case below has max_iter >= 4 * kGraphIters = 64, so whole chunks of 16 iterations are
    replayed from one captured graph (if the runtime declines the capture the same kernels are launched directly: the
    library does not say which happened, so this case proves the record under replay only where capture works)."""
    st = _store()
    o = c_oracle.Store(st.row_ptr, st.tid, st.as_prob, None, T)
    cases = [(1000, 1e-3, 50, False), (1000, 1e-2, 1, True), (70, 0.0, 50, False)]
    if how == "caller_order":
        with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, T, reorder_rows=1) as d:
            _cases_on(d, o, st, how, cases)
        return
    monkeypatch.setenv("OEM_DEFERRED_RELDIFF" if how == "deferred_off" else "OEM_GRAPH", "0" if how == "deferred_off" else "1")
    with _lib.testing(), DeviceStore(st.row_ptr, st.tid, st.as_prob, None, T) as d:
        _cases_on(d, o, st, how, cases)


@pytest.mark.parametrize("coding", [0, 2])
def test_coverage_stores_record_every_iteration(coding):
    """an f64 weight column, and weight_coding = 2 (the product rounded once to f32); the oracle is given the same
    weights"""
    st = _store(coverage=True)
    assert st.cov_prob is not None
    if coding == 2:
        w32 = (st.as_prob.astype(np.float64) * st.cov_prob).astype(np.float32)
        o = c_oracle.Store(st.row_ptr, st.tid, w32, None, T)
    else:
        o = c_oracle.Store(st.row_ptr, st.tid, st.as_prob, st.cov_prob, T)
    with DeviceStore(st.row_ptr, st.tid, st.as_prob, st.cov_prob, T, weight_coding=coding) as d:
        _cases_on(d, o, st, f"coverage, weight_coding {coding}", CASES[:1])


def _free_port():
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 3])
def test_row_shards_record_the_same_history_on_every_rank(world, tmp_path):
    """processes that share the one device, peer-to-peer exchange fused into the rel-diff kernel
    (tests/mp/run_history_worker.py): bitwise identical on every rank, the oracle's within the tolerance, the length of
    the un-sharded run.  The children run under their own timeout; a failed child ends the test."""
    out = tmp_path / "hist.json"
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = ["timeout", "-k", "10", "420", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node",
           str(world), "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "mp", "run_history_worker.py"), str(out)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=480)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    rep = json.load(open(out))
    assert rep["ok"] and rep["world"] == world, rep


@pytest.mark.timeout(300)
def test_row_shards_over_the_process_local_communicator():
    """ranks as threads of this process (test-only library): the exchange is a separate all-reduce and the record is
    written by k_reldiff_swap_clear"""
    world = 2
    st = _store()
    o = c_oracle.Store(st.row_ptr, st.tid, st.as_prob, None, T)
    with _lib.testing():
        handles = (C.c_void_p * world)()
        _lib.check(_lib.lib().oem_debug_local_comm_create(world, 0, C.addressof(handles)))
        res, errs = [None] * world, []

        def rank_main(rank):
            try:
                sh = odist.shard_rows_by_nnz(st.row_ptr, st.tid, st.as_prob, None, rank, world)
                with DeviceStore(sh.row_ptr, sh.tid, sh.as_prob, None, T) as d:
                    d.attach_comm(C.c_void_p(handles[rank]), st.n_reads, sh.row_begin)
                    d.set_option(_lib.OEM_OPT_RUN_HISTORY, 400)
                    _cnt, info = d.em_run(None, 400, 1e-3, 50)
                    res[rank] = (info, d.run_history(0), d.run_history_len(0))
            except Exception as e:  # pragma: no cover
                errs.append((rank, repr(e)))

        th = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=240)
        for h in handles:
            _lib.lib().oem_comm_destroy(C.c_void_p(h))
    assert not errs and all(r is not None for r in res), errs
    want = oracle_history(o, st.n_reads, None, 400, 1e-3, 50)
    _, wi = c_oracle.do_em(o, max_iter=400, conv_thresh=1e-3)
    assert (want[1], want[2]) == (wi.niter, wi.converged)
    for r in range(world):
        assert res[r][1].tobytes() == res[0][1].tobytes(), f"rank {r} differs from rank 0"
        check_history(res[r][1], res[r][2], res[r][0], want, f"process-local rank {r}")


def _resamples(n_boot, n_reads, seed=2):
    rng = np.random.default_rng(seed)
    return np.stack([np.bincount(rng.integers(0, n_reads, n_reads), minlength=n_reads)
                     for _ in range(n_boot)]).astype(np.uint32)


def _check_bootstrap(d, o, st, W, max_iter, thresh, what, batch=True):
    n_boot = len(W)
    d.set_option(_lib.OEM_OPT_BATCH_BOOTSTRAP, 1 if batch else 0)
    d.set_option(_lib.OEM_OPT_RUN_HISTORY, max_iter)
    _out, infos = d.bootstrap(n_boot, row_w_all=W, max_iter=max_iter, conv_thresh=thresh)
    for b in range(n_boot):
        want = oracle_history(o, st.n_reads, None, max_iter, thresh, 50, row_w=W[b])
        _, wi = c_oracle.do_em(o, row_w=W[b], max_iter=max_iter, conv_thresh=thresh)
        assert (want[1], want[2]) == (wi.niter, wi.converged), (what, b)
        check_history(d.run_history(b), d.run_history_len(b), infos[b], want, f"{what}, replicate {b}")
    with pytest.raises(_lib.OemError) as ei:
        d.run_history_len(n_boot)
    assert ei.value.code == _lib.OEM_ERR_ARG


@pytest.mark.parametrize("how", ["batched", "one_per_pass", "multiplicity_256"])
def test_bootstrap_records_one_history_per_replicate(how):
    """11 injected resamples over 2 chains x 4 slots (slots are reused: a slot's record is copied to its replicate's
    row before the next replicate takes it), the same with OEM_OPT_BATCH_BOOTSTRAP = 0, and with one resample that
    carries a multiplicity of 256 and takes the one-per-pass path between the batched ones."""
    st = _store()
    o = c_oracle.Store(st.row_ptr, st.tid, st.as_prob, None, T)
    W = _resamples(11, st.n_reads)
    if how == "multiplicity_256":
        W[4, :] = 1
        W[4, 11] = 256
        W[4, 100:355] = 0          # (the resample still holds n_reads reads)
        assert W[4].sum() == st.n_reads
    with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, T) as d:
        _check_bootstrap(d, o, st, W, 150, 1e-3, how, batch=(how != "one_per_pass"))


def test_device_drawn_bootstrap_records_against_the_reference_stream():
    st = _store()
    o = c_oracle.Store(st.row_ptr, st.tid, st.as_prob, None, T)
    n_boot, seed, max_iter = 5, 99, 120
    with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, T) as d:
        d.set_option(_lib.OEM_OPT_RUN_HISTORY, max_iter)
        _out, infos = d.bootstrap(n_boot, seed=seed, max_iter=max_iter, conv_thresh=1e-3)
        for b in range(n_boot):
            w = resample_np.bootstrap_weights(st.n_reads, seed, b)
            want = oracle_history(o, st.n_reads, None, max_iter, 1e-3, 50, row_w=w)
            check_history(d.run_history(b), d.run_history_len(b), infos[b], want, f"device-drawn replicate {b}")


def test_capacity_bounds_what_is_stored_not_what_is_counted():
    st = _store()
    K, max_iter = 7, 80
    L = _lib.lib()
    with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, T) as d:
        d.set_option(_lib.OEM_OPT_RUN_HISTORY, max_iter)
        _c, full_info = d.em_run(None, max_iter, 1e-3, 50)
        full = d.run_history(0)
        assert len(full) == full_info.niter + int(full_info.converged) > K
        d.set_option(_lib.OEM_OPT_RUN_HISTORY, K)
        _c, info = d.em_run(None, max_iter, 1e-3, 50)
        assert (info.niter, info.converged) == (full_info.niter, full_info.converged)
        assert d.info(_lib.OEM_INFO_RUN_HISTORY_STORED) == K
        guard = np.float64(-12345.678)
        buf = np.full(K + 8, guard)
        n = C.c_uint32(0)
        _lib.check(L.oem_run_history(d.handle, 0, buf.ctypes.data, K + 8, C.byref(n)))
        assert n.value == len(full)                                   # the full count
        assert np.all(buf[K:] == guard)                               # only K entries exist
        for k in range(K):                                            # (not bitwise: the flush atomics' order differs)
            assert close(buf[k], full[k]), (k, buf[k], full[k])
        assert len(d.run_history(0)) == K
        # a caller's buffer smaller than the record: nothing past out[capacity)
        buf = np.full(K, guard)
        _lib.check(L.oem_run_history(d.handle, 0, buf.ctypes.data, 3, C.byref(n)))
        assert n.value == len(full) and np.all(buf[3:] == guard) and all(close(buf[k], full[k]) for k in range(3))
        n.value = 0
        _lib.check(L.oem_run_history(d.handle, 0, None, 0, C.byref(n)))   # the length alone
        assert n.value == len(full)
        assert L.oem_run_history(d.handle, 1, None, 0, C.byref(n)) == _lib.OEM_ERR_ARG
        # K above max_iter: the buffer follows min(K, max_iter)
        d.set_option(_lib.OEM_OPT_RUN_HISTORY, 0xFFFFFFFF)
        _c, info = d.em_run(None, 12, 0.0, 50)
        assert d.info(_lib.OEM_INFO_RUN_HISTORY_STORED) == 12 and len(d.run_history(0)) == 12 == info.niter


def test_off_means_off():
    st = _store()
    L = _lib.lib()
    n = C.c_uint32(0)
    with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, T) as d:
        assert L.oem_run_history(d.handle, 0, None, 0, C.byref(n)) == _lib.OEM_ERR_STATE      # no run yet
        off_cnt, off_info = d.em_run(None, 1000, 1e-3, 50)
        assert L.oem_run_history(d.handle, 0, None, 0, C.byref(n)) == _lib.OEM_ERR_STATE      # the default: off
        assert d.info(_lib.OEM_INFO_RUN_HISTORY_STORED) == 0
        d.set_option(_lib.OEM_OPT_RUN_HISTORY, 1000)
        assert L.oem_run_history(d.handle, 0, None, 0, C.byref(n)) == _lib.OEM_ERR_STATE      # on, but nothing has run
        on_cnt, on_info = d.em_run(None, 1000, 1e-3, 50)
        assert len(d.run_history(0)) == on_info.niter + int(on_info.converged)
        d.set_option(_lib.OEM_OPT_RUN_HISTORY, 0)
        assert L.oem_run_history(d.handle, 0, None, 0, C.byref(n)) == _lib.OEM_ERR_STATE      # a change of the option
        d.em_run(None, 1000, 1e-3, 50)
        assert L.oem_run_history(d.handle, 0, None, 0, C.byref(n)) == _lib.OEM_ERR_STATE
        d.set_option(_lib.OEM_OPT_RUN_HISTORY, 100)
        d.bootstrap(3, seed=1, max_iter=60)
        assert d.run_history_len(2) >= 52
        d.em_run(None, 0, 1e-3, 50)                                                            # a run without iterations
        assert d.run_history_len(0) == 0 and len(d.run_history(0)) == 0
    assert (on_info.niter, on_info.converged) == (off_info.niter, off_info.converged)
    assert_counts_close(on_cnt, off_cnt, st.n_reads, T, 1e-9, "recording on against off")


@pytest.mark.timeout(900)
def test_one_mid_size_run():
    """BASELINE configs[1] (1 M reads x 60 k transcripts), 1000 iterations without early exit as
    tests/test_gpu_parity.py::test_full_size_properties spends on that shape: the record where the deferred rel-diff
    workgroups and the fold share the device."""
    st = synth.make_config("c2")
    o = c_oracle.Store(st.row_ptr, st.tid, st.as_prob, None, st.n_txps)
    with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, st.n_txps) as d:
        d.set_option(_lib.OEM_OPT_RUN_HISTORY, 1000)
        _cnt, info = d.em_run(None, 1000, 0.0, 50)
        got, n = d.run_history(0), d.run_history_len(0)
    assert info.niter == 1000 and not info.converged
    want = oracle_history(o, st.n_reads, None, 1000, 0.0, 50)
    check_history(got, n, info, want, "c2, 1000 iterations")
