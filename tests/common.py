"""Shared helpers of the test-suite (tests are the only place oracle/ is used)."""
import glob
import os

import numpy as np

from oarfish_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    d = {k: z[k] for k in z.files}
    d["n_txps"] = int(d["n_txps"][0])
    d.setdefault("cov_prob", None)
    d.setdefault("init", None)
    runs = []
    n = 0
    while f"run{n}_params" in d:
        mi, ct, gate = d[f"run{n}_params"]
        niter, npass, conv, rel = d[f"run{n}_info"]
        runs.append(dict(max_iter=int(mi), conv_thresh=float(ct), gate=int(gate), counts=d[f"run{n}_counts"],
                         niter=int(niter), n_passes=int(npass), converged=bool(conv), rel_diff=float(rel)))
        n += 1
    d["runs"] = runs
    return d


def assert_counts_close(got, want, n_reads, n_txps, rtol=1e-4, what=""):
    """BASELINE.json north_star: abundances match to <= 1e-4 relative.
    |a-b| <= rtol * max(|b|, 1e-5 * R/T) avoids 0/0 on absent transcripts."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    floor = 1e-5 * max(n_reads, 1) / max(n_txps, 1)
    tol = rtol * np.maximum(np.abs(want), floor)
    bad = np.abs(got - want) > tol
    assert not bad.any(), (
        f"{what}: {bad.sum()} of {len(want)} transcripts differ; worst rel "
        f"{np.max(np.abs(got - want) / np.maximum(np.abs(want), floor)):.3e}")


def weights_with(n_distinct, size, rng):
    vals = ((1.0 + np.arange(n_distinct)) / (n_distinct + 3.0)).astype(np.float32)
    p = vals[rng.integers(0, n_distinct, size=size)]
    p[:n_distinct] = vals
    return p


def tile_test_store(kind, seed):
    """(row_ptr, tid, as_prob, n_txps) of the shapes the tile kernels are tested on."""
    rng = np.random.default_rng(seed)
    if kind == "dense":        # many reads per transcript: hot anchors, 8 window copies
        st = synth.make_store(150_000, 2_000, seed=seed)
    elif kind == "sparse":     # wide windows, few reads per tile window entry
        st = synth.make_store(60_000, 40_000, seed=seed)
    elif kind == "long":       # reads with 20+ local alignments: the reload loops behind the register sets
        st = synth.make_store(30_000, 3_000, kbar=24.0, seed=seed)
    elif kind == "remote":     # mostly-remote: more records than a thread's six register slots (overflow path)
        n, T = 40_000, 30_000
        k = rng.integers(6, 14, n)
        row_ptr = np.concatenate([[0], np.cumsum(k)]).astype(np.uint64)
        tid = np.empty(int(row_ptr[-1]), np.uint32)
        for i in range(n):     # distinct transcripts per read, all over the annotation
            tid[int(row_ptr[i]):int(row_ptr[i + 1])] = rng.choice(T, int(k[i]), replace=False)
        p = np.exp(-rng.integers(0, 30, len(tid)) / 5.0).astype(np.float32)
        return row_ptr, tid, p, T
    elif kind == "tiny":       # one tile, three slices
        st = synth.make_store(150, 40, seed=seed)
    elif kind == "ragged":     # a last tile with a few reads, single-alignment reads, one very long read
        st = synth.make_store(20_000 + 7, 900, seed=seed)
    else:
        raise ValueError(kind)
    return st.row_ptr, st.tid, st.as_prob, st.n_txps


def byte_edge_weights(n_reads, seed):
    """Injected resamples around the batched bootstrap's byte-coded multiplicities (a replicate with a multiplicity
    >= 256 must be handed to the one-per-pass path; 255 must still be exact in a byte).  Returns (row_w_all u32[7, R],
    names): ordinary resamples (the device stream's, drawn by the reference) sit between the edge replicates, so that
    a replicate that falls back is handed over in the middle of a running chain.  The reads that carry 255 / 256 are
    spread over the store so that they land in different tiles."""
    from oracle import resample_np
    W = np.stack([resample_np.bootstrap_weights(n_reads, seed, b) for b in range(7)])
    at = lambda f: int(f * (n_reads - 1))   # noqa: E731
    W[1, [at(0.1), at(0.5), at(0.9)]] = 255
    W[3, at(0.3)] = 256
    W[4, [at(0.2), at(0.7)]] = (255, 256)
    k = max(n_reads // 200, 1)
    W[5] = 0
    W[5, :k] = 255
    names = ["ordinary", "a few at 255", "ordinary", "one at 256", "255 and 256", "all 255 on the first reads",
             "ordinary"]
    return W.astype(np.uint32), names


def f32_ulps(a, b):
    """Distance in f32 units in the last place between two f32 arrays of one sign."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def assert_cell_matches_oracle(info, want_info, n_reads, n_txps, what, dense=None, cols=None, vals=None):
    """One cell of a per-cell EM call against the oracle's em::em on the cell's own store.  The iteration counts are
    at most one apart; `converged` and the number of passes agree when they are equal.  Dense row: within 1e-8 when
    the counts agree, the 1e-4 north star otherwise.  Sparse row (cols, vals): the columns are exactly the oracle's
    v > 0 and each value is within one f32 ulp of the oracle's when the counts agree, the north star otherwise."""
    want, wi = want_info
    assert abs(int(info.niter) - int(wi.niter)) <= 1, (what, info, wi)
    same = info.niter == wi.niter
    if same:
        assert bool(info.converged) == bool(wi.converged) and info.n_passes == wi.n_passes, (what, info, wi)
    if dense is not None:
        assert_counts_close(dense, want, n_reads, n_txps, 1e-8 if same else 1e-4, what)
        return
    got = np.zeros(n_txps)
    got[cols] = vals
    if same:
        np.testing.assert_array_equal(cols, np.nonzero(want > 0.0)[0], err_msg=what)
        ulps = f32_ulps(vals, want[cols].astype(np.float32))
        assert ulps.max(initial=0) <= 1, f"{what}: {int(ulps.max())} f32 ulps from the oracle"
    else:
        assert_counts_close(got, want, n_reads, n_txps, 1e-4, what)
