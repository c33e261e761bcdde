"""What the run-history tests share: the expected rel_diff trajectory of a run, computed from the oracle's single
pass (oracle.c_oracle.m_step) with em.rs:194-218 applied in NumPy, and the checks every recorded run is held to."""
import numpy as np

from oracle import c_oracle

MIN_READ_THRESH = 1e-5


def oracle_history(o, n_reads_total, init=None, max_iter=1000, thresh=1e-3, gate=50, row_w=None):
    """(history, niter, converged) of do_em / em_par on oracle store `o`: history[k] is the rel_diff of loop pass k,
    the value em.rs:194-201 leaves.  rel_diff is discontinuous where a prev_counts[i] sits on MIN_READ_THRESH
    (em.rs:195), so the trajectory is only a reference while no prev_counts[i] comes within 1e-9 relative of it:
    asserted here at every iteration, so that a change of seed cannot hide behind it."""
    T = o.n_txps
    prev = np.full(T, n_reads_total / T) if init is None else np.array(init, dtype=np.float64)   # em.rs:160-167
    hist, niter, converged = [], 0, False
    while niter < max_iter:                                                                        # em.rs:181
        curr = c_oracle.m_step(o, prev, row_w=row_w)
        edge = np.abs(prev - MIN_READ_THRESH) <= 1e-9 * MIN_READ_THRESH
        assert not edge.any(), f"iteration {niter}: prev_counts{np.nonzero(edge)[0][:4]} sit on MIN_READ_THRESH"
        m = prev > MIN_READ_THRESH
        rel = 0.0                                                                                  # em.rs:169 / :234
        if m.any():
            rel = max(rel, float(np.max((curr[m] - prev[m]) / prev[m])))                           # em.rs:195-199 (signed)
        hist.append(rel)
        prev = curr                                                                                # em.rs:204
        if rel < thresh and niter > gate:                                                          # em.rs:212 / :399
            converged = True
            break
        niter += 1                                                                                 # em.rs:218
    return np.array(hist, dtype=np.float64), niter, converged


def close(a, b):
    """the tolerance tests/test_gpu_parity.py holds info.rel_diff to"""
    return abs(a - b) <= 1e-9 * max(abs(b), 1e-12) + 1e-15


def check_history(got, n_total, info, want, what):
    """`got`: the stored entries, `n_total`: oem_run_history's out_len, `info`: the run's RunInfo, `want`: the
    oracle loop's (history, niter, converged).  Prints each figure it is about to hold to the tolerance."""
    whist, wniter, wconv = want
    assert (info.niter, bool(info.converged)) == (wniter, wconv), (what, info, wniter, wconv)
    assert n_total == info.niter + int(info.converged) == info.n_passes - 1, (what, n_total, info)
    assert len(whist) == n_total, (what, len(whist), n_total)
    assert len(got) == n_total, (what, len(got), n_total)
    if n_total:
        assert got[-1].tobytes() == np.float64(info.rel_diff).tobytes(), (what, got[-1], info.rel_diff)
    worst = max((abs(a - b) / max(abs(b), 1e-12) for a, b in zip(got, whist)), default=0.0)
    print(f"{what}: {n_total} entries, worst relative deviation {worst:.3e}")
    for k, (a, b) in enumerate(zip(got, whist)):
        assert close(a, b), f"{what}: entry {k}: {a!r} against {b!r}"
