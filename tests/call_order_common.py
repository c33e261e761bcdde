"""What the call-order tests share (tests/test_call_order.py, tests/test_call_order_gpu.py).

An oem_store is a long-lived handle with a lot of lazily allocated, reused state (struct oem_store, oem_internal.h);
the tests here hold that a call's result does not depend on the calls made before it on the same handle.  This module
has the three pieces of that:

  the alphabet   OPS: small named operations `run(d, fx) -> result` on an open DeviceStore.  An operation sets every
                 option and environment knob it depends on and takes the knob away again; it leaves the options as it
                 set them, so the next operation runs under a leftover OEM_OPT_RUN_HISTORY / batch flag / first replica
                 it does not name -- which is part of what is tested.
  the walk       euler_walk(n): n^2 + 1 operation indices in which every ordered pair, self pairs included, occurs as
                 neighbours exactly once (an Eulerian circuit of the complete digraph with loops, Hierholzer).
  the references oracle_ref(store, op): the operation on the f64 oracle, history-free by construction; fresh_ref(...):
                 the same operation as the first call on a fresh handle.  hold(...) holds one result to both.

Stores (tests/common.tile_test_store, seed 23): A = "remote" (40 000 reads, 30 000 transcripts: several tiles, 8
buckets, more remote records than register slots, generator weights with the fused dictionary), B = "long" with a
coverage column (f64 weights, the reload loops).

Tolerances.  Against the oracle the project's own: one pass 1e-10, a 40-iteration run with equal niter 1e-9, converged
runs and replicates with equal niter 1e-8, |sum - R| < 1e-7 R, aux_counts exact, assignment_probs 1e-12 with equal
kept sets.  Against the fresh handle: exact for everything integral or bit-stable (aux_counts, bootstrap_weights,
assignment_probs, text bytes, line_off, kept, the lz4 frame, niter, n_passes, converged, run_history_len), 1e-6
relative for recorded rel_diff values (the golden-fixture allowance), 1e-12 for one-pass counts (the project's number
for two atomic orders of the same sums), and for multi-iteration counts ten times the run-to-run noise measured
between two fresh handles (fresh_ref: only two samples are measured, and the order of the atomics varies), never above
the operation's oracle tolerance.

Stopping must be exact, so the inputs keep the oracle off the knife-edge: THRESH = 1e-2, and stopping_margins() gives
what tests/test_call_order.py asserts -- every converging run of the alphabet stops between the gate and max_iter with
its rel_diff at least MARGIN * THRESH away from THRESH at the stopping iteration and at the one before (100 times the
1e-6 the suite allows between device and oracle rel_diff)."""
import contextlib
import functools
import os
import tempfile
from dataclasses import dataclass
from typing import Callable, Tuple

import numpy as np

from oarfish_amd import _lib
from oarfish_amd.types import DeviceStore
from oracle import c_oracle, resample_np
from tests.common import assert_counts_close, byte_edge_weights, tile_test_store
from tests.run_history_common import oracle_history

THRESH = 1e-2
MARGIN = 1e-4            # of THRESH
N_ITER, MAX_ITER, GATE = 40, 200, 50
STORES = ("A", "B")
SEED_DRAWN, FIRST_DRAWN, N_DRAWN = 99, 3, 3       # the device-drawn bootstrap: replicas 3, 4, 5 of stream 99
SEED_WEIGHTS, REPLICA_WEIGHTS = 7, 2              # bootstrap_weights
ONE_PASS_TOL = 1e-12
HISTORY_RTOL = 1e-6
PREFIX = b"2\t1\nT0\nT1\n"                        # (any bytes: the header lines of the .prob file)


# ---- the walk -----------------------------------------------------------------------------------------------------------
def euler_walk(n):
    """n^2 + 1 vertices of an Eulerian circuit of the complete digraph on n vertices with loops (Hierholzer): every
    ordered pair (a, b), a == b included, is a pair of neighbours exactly once.  Starts and ends at 0."""
    nxt = [0] * n                     # vertex v has used its edges to 0 .. nxt[v] - 1
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < n:
            stack.append(nxt[v])
            nxt[v] += 1
        else:
            out.append(stack.pop())
    return out[::-1]


# ---- stores and inputs (computed once, shared, never written to) ---------------------------------------------------------
class Fixture:
    pass


@functools.lru_cache(maxsize=None)
def fixture(store):
    fx = Fixture()
    fx.store = store
    row_ptr, tid, p, T = tile_test_store({"A": "remote", "B": "long"}[store], 23)
    cov = np.random.default_rng(77).uniform(1e-3, 1.0, len(tid)) if store == "B" else None
    R = len(row_ptr) - 1
    fx.row_ptr, fx.tid, fx.p, fx.cov, fx.T, fx.R = row_ptr, tid, p, cov, T, R
    rng = np.random.default_rng(5)
    theta = rng.lognormal(0.0, 1.5, T)
    theta[rng.random(T) < 0.1] = 0.0
    fx.theta = theta                                          # m_step's argument and em_init's init_abundances: 10 % zeros
    fx.row_w = rng.poisson(1.0, size=R).astype(np.uint32)
    fx.boot_w = rng.multinomial(R, np.full(R, 1.0 / R), size=5).astype(np.uint32)      # 5 > the 4 slots of one chain
    # init_abundances of the bootstrap that takes one: spread around the uniform start, no zeros (from the vector above
    # two of six replicates of store A would still be running at max_iter)
    fx.boot_init = np.random.default_rng(3).lognormal(0.0, 0.5, T) * R / T
    fx.init_w = np.random.default_rng(6).multinomial(R, np.full(R, 1.0 / R), size=6).astype(np.uint32)
    assert fx.boot_w.max() < 256 and fx.init_w.max() < 256
    fx.edge_w, fx.edge_names = byte_edge_weights(R, 11)
    fx.drawn_w = np.stack([resample_np.bootstrap_weights(R, SEED_DRAWN, FIRST_DRAWN + b) for b in range(N_DRAWN)])
    assert fx.drawn_w.max() < 256
    fx.names = [f"read/{i:x}" + "#" * (i % 5) for i in range(R)]
    fx.o = c_oracle.Store(row_ptr, tid, p, cov, T)
    fx.counts, info = c_oracle.do_em(fx.o, max_iter=MAX_ITER, conv_thresh=THRESH, min_iter_gate=GATE)
    assert info.converged
    for a in (theta, fx.boot_init, fx.row_w, fx.boot_w, fx.init_w, fx.edge_w, fx.drawn_w, fx.counts):
        a.setflags(write=False)
    return fx


def open_store(fx):
    """A fresh handle in the library in use (inside `_lib.testing()`: the test-only one)."""
    return DeviceStore(fx.row_ptr, fx.tid, fx.p, fx.cov, fx.T)


# the converging runs of the alphabet: (what, replicates' multiplicities or None for the point estimate, init or None)
def converging_runs(fx):
    runs = [("point estimate (em_converged, em_converged_graph)", None, None)]
    runs += [(f"boot_batched / history_500 replicate {b}", fx.boot_w[b], None) for b in range(len(fx.boot_w))]
    runs += [(f"boot_byte_edge replicate {b} ({fx.edge_names[b]})", fx.edge_w[b], None) for b in range(len(fx.edge_w))]
    runs += [(f"boot_single_drawn replica {FIRST_DRAWN + b}", fx.drawn_w[b], None) for b in range(N_DRAWN)]
    runs += [(f"boot_init replicate {b}", fx.init_w[b], fx.boot_init) for b in range(len(fx.init_w))]
    return runs


def stopping_margins(store):
    """[(what, niter, converged, rel_diff at the stopping iteration, rel_diff at the one before)] of every converging
    run, from the oracle's own trajectory (run_history_common.oracle_history)."""
    fx = fixture(store)
    out = []
    for what, w, init in converging_runs(fx):
        hist, niter, conv = oracle_history(fx.o, fx.R, init, MAX_ITER, THRESH, GATE, row_w=w)
        out.append((what, niter, conv, float(hist[-1]), float(hist[-2])))
    return out


# ---- the alphabet ----------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _env(**kv):
    """environment knobs of the test-only library, set for the block and taken away again"""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _runs(counts, infos):
    return {"counts": np.atleast_2d(counts), "infos": list(infos)}


def _run(d, init, max_iter, thresh):
    c, i = d.em_run(init, max_iter, thresh, GATE)
    return _runs(c, [i])


def _boot(d, batched, W, init=None, chains=None):
    d.set_option(_lib.OEM_OPT_BATCH_BOOTSTRAP, batched)
    with _env(**({"OEM_BOOT_CHAINS": str(chains)} if chains else {})):
        out, infos = d.bootstrap(len(W), row_w_all=W, init=init, max_iter=MAX_ITER, conv_thresh=THRESH)
    return _runs(out, infos)


def op_m_step(d, fx):
    return {"counts": d.m_step(fx.theta)[None]}


def op_m_step_weighted(d, fx):
    return {"counts": d.m_step(fx.theta, fx.row_w)[None]}


def op_em_40(d, fx):                    # reaches max_iter: the deferred loop ends in k_deferred_sweep
    return _run(d, None, N_ITER, 0.0)


def op_em_converged(d, fx):             # the speculative pass is dropped, `done` is set
    return _run(d, None, MAX_ITER, THRESH)


def op_em_init(d, fx):
    return _run(d, fx.theta, N_ITER, 0.0)


def op_em_zero(d, fx):
    return _run(d, None, 0, THRESH)


def op_em_40_classic(d, fx):
    with _env(OEM_DEFERRED_RELDIFF="0"):
        return _run(d, None, N_ITER, 0.0)


def op_em_converged_graph(d, fx):
    with _env(OEM_GRAPH="1"):
        return _run(d, None, MAX_ITER, THRESH)


def op_boot_batched(d, fx):             # one chain: four start, the fifth goes to the slot that finishes first
    return _boot(d, 1, fx.boot_w, chains=1)


def op_boot_byte_edge(d, fx):           # a replicate at 256 is handed to the one-per-pass path in the middle of a chain
    return _boot(d, 1, fx.edge_w, chains=1)


def op_boot_single_drawn(d, fx):
    d.set_option(_lib.OEM_OPT_BATCH_BOOTSTRAP, 0)
    out, infos = d.bootstrap(N_DRAWN, seed=SEED_DRAWN, max_iter=MAX_ITER, conv_thresh=THRESH, first_replica=FIRST_DRAWN)
    return _runs(out, infos)


def op_boot_init(d, fx):                # default chains: two chains share the init parked in s->theta
    return _boot(d, 1, fx.init_w, init=fx.boot_init)


def op_aux_counts(d, fx):
    u, t = d.aux_counts()
    return {"exact": {"unique": u, "total": t}}


def op_assignment_probs(d, fx):
    return {"exact": {"probs": d.assignment_probs(fx.counts, 1e-3)}}


def _text(res):
    return {"text": res.text.tobytes(), "line_off": res.line_off, "kept": res.kept}


def op_assignment_text(d, fx):
    return {"exact": _text(d.assignment_text(fx.counts, 1e-6, fx.names))}


def op_assignment_text_lz4(d, fx):
    res = d.assignment_text_lz4(fx.counts, 0.2, fx.names, PREFIX)
    ex = _text(res)
    ex.update(content_bytes=res.content_bytes, n_blocks=res.n_blocks, raw_blocks=res.raw_blocks)
    return {"exact": ex}


def op_bootstrap_weights(d, fx):
    return {"exact": {"w": d.bootstrap_weights(SEED_WEIGHTS, REPLICA_WEIGHTS)}}


def _with_history(d, res):
    n = len(res["infos"])
    res["hist"] = [d.run_history(b) for b in range(n)]
    res.setdefault("exact", {})["run_history_len"] = [d.run_history_len(b) for b in range(n)]
    return res


def op_history_8(d, fx):
    d.set_option(_lib.OEM_OPT_RUN_HISTORY, 8)
    return _with_history(d, op_em_40(d, fx))


def op_history_500(d, fx):              # the buffers regrow
    d.set_option(_lib.OEM_OPT_RUN_HISTORY, 500)
    res = _with_history(d, op_boot_batched(d, fx))
    d.set_option(_lib.OEM_OPT_RUN_HISTORY, 0)
    return res


def op_time_m_step(d, fx):              # leaves cnt non-zero on purpose
    assert d.time_m_step(3) > 0.0
    return {}


def op_time_em_iters(d, fx):
    assert d.time_em_iters(7) > 0.0
    return {}


def op_time_bootstrap_passes(d, fx):    # leaves four slots RUNNING
    ms, slots, nbytes = d.time_bootstrap_passes(3)
    assert ms > 0.0 and slots > 0 and nbytes > 0
    return {}


def op_err_option(d, fx):               # rejected on the host before any device work
    rc = d._lib.oem_store_set_option(d.handle, 99, 1)
    assert rc == _lib.OEM_ERR_ARG, rc
    return {}


def op_err_replica(d, fx):              # first_replica + n_boot passes 2^32 - 1: rejected on the host
    try:
        d.bootstrap(3, seed=1, max_iter=MAX_ITER, conv_thresh=THRESH, first_replica=0xFFFFFFFE)
    except _lib.OemError as e:
        assert e.code == _lib.OEM_ERR_ARG, e
    else:
        raise AssertionError("oem_bootstrap accepted replicas past 2^32 - 1")
    return {}


@dataclass(frozen=True)
class Op:
    name: str
    run: Callable
    knobs: Tuple[str, ...] = ()         # environment knobs of the test-only library the operation sets
    kind: str = "state"                 # "pass", "run40", "converged" (its oracle tolerance), or "exact" / "state"


OPS = [
    Op("m_step", op_m_step, kind="pass"),
    Op("m_step_weighted", op_m_step_weighted, kind="pass"),
    Op("em_40", op_em_40, kind="run40"),
    Op("em_converged", op_em_converged, kind="converged"),
    Op("em_init", op_em_init, kind="run40"),
    Op("em_zero", op_em_zero, kind="pass"),
    Op("em_40_classic", op_em_40_classic, ("OEM_DEFERRED_RELDIFF",), "run40"),
    Op("em_converged_graph", op_em_converged_graph, ("OEM_GRAPH",), "converged"),
    Op("boot_batched", op_boot_batched, ("OEM_BOOT_CHAINS",), "converged"),
    Op("boot_byte_edge", op_boot_byte_edge, ("OEM_BOOT_CHAINS",), "converged"),
    Op("boot_single_drawn", op_boot_single_drawn, kind="converged"),
    Op("boot_init", op_boot_init, kind="converged"),
    Op("aux_counts", op_aux_counts, kind="exact"),
    Op("assignment_probs", op_assignment_probs, kind="exact"),
    Op("assignment_text", op_assignment_text, kind="exact"),
    Op("assignment_text_lz4", op_assignment_text_lz4, kind="exact"),
    Op("bootstrap_weights", op_bootstrap_weights, kind="exact"),
    Op("history_8", op_history_8, kind="run40"),
    Op("history_500", op_history_500, ("OEM_BOOT_CHAINS",), "converged"),
    Op("time_m_step", op_time_m_step),
    Op("time_em_iters", op_time_em_iters),
    Op("time_bootstrap_passes", op_time_bootstrap_passes),
    Op("err_option", op_err_option),
    Op("err_replica", op_err_replica),
]
BY_NAME = {op.name: op for op in OPS}
KNOB_FREE = [op for op in OPS if not op.knobs]                # what the product library can run as written
ORACLE_TOL = {"pass": 1e-10, "run40": 1e-9, "converged": 1e-8}

# The pairs the code makes riskiest, then every pair the walk found broken (with its fix).
PAIRS = [
    ("time_m_step", "m_step"),                   # cnt left non-zero: oem_m_step's own memset
    ("time_em_iters", "em_init"),                # a finished loop state and rotated buffers under an uploaded init
    ("time_bootstrap_passes", "boot_batched"),   # four slots left RUNNING
    ("em_converged", "m_step"),                  # `done` set, a dropped speculative accumulator
    ("m_step_weighted", "m_step"),               # a stale row_w_perm
    ("boot_byte_edge", "boot_batched"),          # a slot's byte column after a replicate that fell back
    ("history_8", "history_500"),                # the history buffers regrow
    ("boot_init", "em_40"),                      # init parked in s->theta
    ("assignment_text", "em_zero"),              # s->theta as scratch for counts
]


# ---- references -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_ref(store, name):
    """The operation on the oracle: {"counts": (n, T), "infos": [RunInfo] or None, "target": mass per run} for the
    float operations, {"exact": {...}} for those the oracle gives exactly, None where the fresh handle's own checks are
    the reference (text: the Python writer on the device's probabilities; lz4: the decoded frame)."""
    fx = fixture(store)
    o = fx.o

    def runs(W, init, max_iter, thresh):
        cs, infos, targets = [], [], []
        for w in ([None] if W is None else W):
            c, i = c_oracle.do_em(o, init=init, max_iter=max_iter, conv_thresh=thresh, min_iter_gate=GATE, row_w=w)
            cs.append(c)
            infos.append(i)
            targets.append(float(fx.R if w is None else w.sum(dtype=np.uint64)))
        return {"counts": np.stack(cs), "infos": infos, "target": targets}

    if name == "m_step":
        return {"counts": c_oracle.m_step(o, fx.theta)[None], "infos": None}
    if name == "m_step_weighted":
        return {"counts": c_oracle.m_step(o, fx.theta, row_w=fx.row_w)[None], "infos": None}
    if name in ("em_40", "em_40_classic", "history_8"):
        ref = runs(None, None, N_ITER, 0.0)
        assert ref["infos"][0].niter == N_ITER
        return ref
    if name in ("em_converged", "em_converged_graph"):
        return runs(None, None, MAX_ITER, THRESH)
    if name == "em_init":
        return runs(None, fx.theta, N_ITER, 0.0)
    if name == "em_zero":
        return runs(None, None, 0, THRESH)
    if name in ("boot_batched", "history_500"):
        return runs(fx.boot_w, None, MAX_ITER, THRESH)
    if name == "boot_byte_edge":
        return runs(fx.edge_w, None, MAX_ITER, THRESH)
    if name == "boot_single_drawn":
        return runs(fx.drawn_w, None, MAX_ITER, THRESH)        # oracle/resample_np.py's stream
    if name == "boot_init":
        return runs(fx.init_w, fx.boot_init, MAX_ITER, THRESH)
    if name == "aux_counts":
        u, t = c_oracle.aux_counts(o)
        return {"exact": {"unique": u, "total": t}}
    if name == "assignment_probs":
        return {"probs": c_oracle.assignment_probs(o, fx.counts, 1e-3)}
    if name == "bootstrap_weights":
        return {"exact": {"w": resample_np.bootstrap_weights(fx.R, SEED_WEIGHTS, REPLICA_WEIGHTS)}}
    return None


def worst_metric(got, want, n_reads, n_txps):
    """assert_counts_close's figure: the worst |a - b| / max(|b|, 1e-5 R / T)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    floor = 1e-5 * max(n_reads, 1) / max(n_txps, 1)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), floor), initial=0.0))


def _equal(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    return a == b


def hold_to_oracle(res, op, fx, what):
    ref = oracle_ref(fx.store, op.name)
    if ref is None:
        return
    for k, want in ref.get("exact", {}).items():
        assert _equal(res["exact"][k], want), f"{what}: {k} differs from the oracle's"
    if "probs" in ref:
        got, want = res["exact"]["probs"], ref["probs"]
        assert np.array_equal(got >= 0, want >= 0), f"{what}: kept sets differ from the oracle's"
        assert np.max(np.abs(got - want), initial=0.0) <= 1e-12, f"{what}: assignment_probs against the oracle"
    if "counts" in ref:
        tol = ORACLE_TOL[op.kind]
        assert res["counts"].shape == ref["counts"].shape, (what, res["counts"].shape)
        for b in range(len(ref["counts"])):
            if ref["infos"] is not None:
                gi, wi = res["infos"][b], ref["infos"][b]
                assert (gi.niter, bool(gi.converged)) == (wi.niter, bool(wi.converged)), (what, b, gi, wi)
            assert_counts_close(res["counts"][b], ref["counts"][b], fx.R, fx.T, tol, f"{what}: run {b} against the oracle")
            if ref["infos"] is not None:
                target = ref["target"][b]
                # (a read whose transcripts all sit at zero drops out of the oracle's sum too: then there is no mass to hold)
                if abs(ref["counts"][b].sum() - target) < 1e-9 * target:
                    assert abs(res["counts"][b].sum() - target) < 1e-7 * target, (what, b, res["counts"][b].sum(), target)


WORST = {}      # (store, operation) -> the worst figure a used handle showed against the fresh one (printed by the walks)


def hold_to_fresh(res, fresh, op, fx, what):
    """`fresh` = fresh_ref(...)[op.name]: (result of the first call on a fresh handle, measured floor, tolerance)."""
    want, _floor, tol = fresh
    assert set(res) == set(want), (what, sorted(res), sorted(want))
    for k, w in want.get("exact", {}).items():
        assert _equal(res["exact"][k], w), f"{what}: {k} differs from the fresh handle's"
    for b, wi in enumerate(want.get("infos", [])):
        gi = res["infos"][b]
        assert (gi.niter, gi.n_passes, bool(gi.converged)) == (wi.niter, wi.n_passes, bool(wi.converged)), (what, b, gi, wi)
    if "counts" in want:
        assert res["counts"].shape == want["counts"].shape, (what, res["counts"].shape)
        for b in range(len(want["counts"])):
            key = (fx.store, op.name)
            WORST[key] = max(WORST.get(key, 0.0), worst_metric(res["counts"][b], want["counts"][b], fx.R, fx.T))
            assert_counts_close(res["counts"][b], want["counts"][b], fx.R, fx.T, tol, f"{what}: run {b} against a fresh handle")
    for b, wh in enumerate(want.get("hist", [])):
        gh = res["hist"][b]
        assert len(gh) == len(wh), (what, b, len(gh), len(wh))
        bad = np.abs(gh - wh) > HISTORY_RTOL * np.abs(wh)
        assert not bad.any(), f"{what}: run {b}: recorded rel_diff {np.nonzero(bad)[0][:4]} differ from the fresh handle's"


def hold(res, fresh, op, fx, what):
    hold_to_oracle(res, op, fx, what)
    hold_to_fresh(res, fresh, op, fx, what)


def _check_text_references(d, res, op, fx):
    """What the oracle cannot give: the fresh handle's text against the Python writer on the device's probabilities
    (as tests/test_assignment_text_gpu.py), its lz4 frame decoded by every decoder at hand."""
    from tests import lz4_common
    from tests.test_assignment_text_gpu import python_body
    if op.name == "assignment_text":
        probs = d.assignment_probs(fx.counts, 1e-6)
        with tempfile.TemporaryDirectory() as tmp:
            import pathlib
            want = python_body(pathlib.Path(tmp), fx.row_ptr, fx.tid, probs, fx.names, fx.T, 1e-6)
        assert res["exact"]["text"] == want, "fresh handle: assignment_text differs from the Python writer"
        lo = fx.row_ptr[:-1].astype(np.int64)
        assert np.array_equal(res["exact"]["kept"], np.add.reduceat((probs >= 0).astype(np.int64), lo))
    if op.name == "assignment_text_lz4":
        body = d.assignment_text(fx.counts, 0.2, fx.names)
        f = lz4_common.decode_everywhere(res["exact"]["text"])
        assert f.content == PREFIX + body.text.tobytes(), "fresh handle: the decoded lz4 frame is not prefix + text"
        assert np.array_equal(res["exact"]["line_off"], body.line_off) and np.array_equal(res["exact"]["kept"], body.kept)


def fresh_ref(fx, ops):
    """{name: (result, floor, tol)}: every operation of `ops` as the first call on a fresh handle of the library in
    use, held to the oracle; for the float operations a second fresh handle gives the run-to-run noise `floor` (the
    worst assert_counts_close figure between the two) and `tol` is what a later call on a used handle is allowed."""
    out = {}
    for op in ops:
        with open_store(fx) as d:
            res = op.run(d, fx)
            hold_to_oracle(res, op, fx, f"fresh handle: {op.name} on store {fx.store}")
            if op.name in ("assignment_text", "assignment_text_lz4"):
                _check_text_references(d, res, op, fx)       # (after the operation: the handle is no longer fresh)
        floor, tol = 0.0, 0.0
        if "counts" in res:
            with open_store(fx) as d:
                again = op.run(d, fx)
            floor = max(worst_metric(again["counts"][b], res["counts"][b], fx.R, fx.T) for b in range(len(res["counts"])))
            tol = ONE_PASS_TOL if op.kind == "pass" else min(ORACLE_TOL[op.kind], 10.0 * floor)
            hold_to_fresh(again, (res, floor, ORACLE_TOL[op.kind]), op, fx, f"second fresh handle: {op.name} on store {fx.store}")
            print(f"store {fx.store}, {op.name}: run-to-run floor {floor:.3e}, allowed {tol:.3e}")
        out[op.name] = (res, floor, tol)
    return out


def walk(d, fx, ops, fresh, executed):
    """Generator: the Euler walk over `ops` on the open handle `d`, one step per next(); every step's result is held
    to its references, a failure names (step, previous operation, operation, store); `executed` collects the pairs."""
    prev = None
    for i, k in enumerate(euler_walk(len(ops))):
        op = ops[k]
        what = f"step {i}: {ops[prev].name if prev is not None else '(fresh)'} -> {op.name} on store {fx.store}"
        try:
            res = op.run(d, fx)
        except Exception as e:
            raise AssertionError(f"{what}: {e!r}") from e
        hold(res, fresh[op.name], op, fx, what)
        if prev is not None:
            executed.add((prev, k))
        prev = k
        yield i


def run_pair(store, a, b, fresh):
    """`a` then `b` on a fresh handle of store `store`, both held to their references."""
    fx = fixture(store)
    with open_store(fx) as d:
        for name, what in ((a, f"(fresh) -> {a}"), (b, f"{a} -> {b}")):
            op = BY_NAME[name]
            hold(op.run(d, fx), fresh[name], op, fx, f"{what} on store {store}")
