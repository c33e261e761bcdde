#!/usr/bin/env python3
"""Times the per-cell EM with its dense result (em_cells: n_cells x n_txps f64) against the sparse one (em_cells_sparse:
the v > 0 f32 entries as CSR, picked out on the device), end to end from host buffers, the faster of two calls of each
(as bench.py's cells leg).  Two workloads: the 625 x 50 k-read slice of one GPU of BASELINE configs[4] (60 k
transcripts), and 1 000 x 20 k-read cells over a 250 k-transcript annotation with 5 % of it expressed per cell.
Prints one JSON line per workload.
usage: cells_sparse_bench.py [slice|annotation ...]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oarfish_amd  # noqa: E402
from oarfish_amd import synth  # noqa: E402

WORKLOADS = {
    "slice": dict(n_cells=625, per_cell=50_000, T=60_000, seed=37, expressed_frac=None),
    "annotation": dict(n_cells=1_000, per_cell=20_000, T=250_000, seed=41, expressed_frac=0.05),
}


def one(name, w):
    threads = min(16, os.cpu_count() or 4)
    cell_off, row_ptr, tid, p = synth.make_cells(w["n_cells"], w["per_cell"], w["T"], seed=w["seed"], threads=threads,
                                                 expressed_frac=w["expressed_frac"])
    T, n = w["T"], w["n_cells"]
    c2 = int(cell_off[2]); a2 = int(row_ptr[c2])
    # HIP runtime start-up and both paths' first use outside the timed calls
    oarfish_amd.em_cells(cell_off[:3], row_ptr[:c2 + 1], tid[:a2], p[:a2], None, T, max_iter=5)
    oarfish_amd.em_cells_sparse(cell_off[:3], row_ptr[:c2 + 1], tid[:a2], p[:a2], None, T, max_iter=5)
    runs = {"dense": [], "sparse": []}
    entries = None
    for _rep in range(2):   # interleaved: a slow spell of the host hits both
        t = time.perf_counter()
        out, _ = oarfish_amd.em_cells(cell_off, row_ptr, tid, p, None, T, max_iter=1000, convergence_thresh=1e-3)
        runs["dense"].append(time.perf_counter() - t)
        dense_nz = int(np.count_nonzero(out > 0.0))
        del out
        t = time.perf_counter()
        indptr, cols, vals, _ = oarfish_amd.em_cells_sparse(cell_off, row_ptr, tid, p, None, T, max_iter=1000,
                                                            convergence_thresh=1e-3)
        runs["sparse"].append(time.perf_counter() - t)
        entries = len(cols)
        del indptr, cols, vals
    best = {k: min(v) for k, v in runs.items()}
    line = {
        "workload": name, "n_cells": n, "reads_per_cell": w["per_cell"], "n_txps": T,
        "expressed_frac": w["expressed_frac"],
        "dense_s": round(best["dense"], 4), "sparse_s": round(best["sparse"], 4),
        "dense_cells_per_s": round(n / best["dense"], 1), "sparse_cells_per_s": round(n / best["sparse"], 1),
        "dense_runs_s": [round(x, 4) for x in runs["dense"]], "sparse_runs_s": [round(x, 4) for x in runs["sparse"]],
        "dense_result_bytes": n * T * 8, "sparse_result_bytes": 8 * (n + 1) + 8 * entries,
        "entries": entries, "dense_nonzeros": dense_nz, "nonzero_frac": round(entries / (n * T), 4),
    }
    print(json.dumps(line), flush=True)


def main():
    names = sys.argv[1:] or list(WORKLOADS)
    for name in names:
        one(name, WORKLOADS[name])


if __name__ == "__main__":
    main()
