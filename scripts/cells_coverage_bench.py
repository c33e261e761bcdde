#!/usr/bin/env python3
"""Times the per-cell coverage model of a single-cell run on the 625 x 50 k-read slice of one GPU of BASELINE
configs[4] (60 k transcripts, coordinates from synth.make_coordinates), end to end from host buffers, each the faster
of two calls after a warm-up:

  batched   cells_coverage_probs (oem_coverage_probs_cells_device): all cells in one call
  loop      oem_coverage_probs_device on each cell's slice, cell after cell (what a caller had before)
  em        em_cells_sparse on the resulting coverage column (the step the coverage model feeds)

The batched result is checked against the loop on every cell.  Writes the JSON line to
profiles/cells_coverage_bench.json (or the path given with --out) and prints it.

usage: cells_coverage_bench.py [--out PATH] [--batched-only]
  --batched-only   generate, warm up and make one batched call, nothing else (the rocprofv3 trace run)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oarfish_amd  # noqa: E402
from oarfish_amd import _lib, synth  # noqa: E402

N_CELLS, READS, T, SEED = 625, 50_000, 60_000, 37


def per_cell_loop(cell_off, row_ptr, tid, s, e, tl, out):
    L = _lib.lib()
    for c in range(len(cell_off) - 1):
        r0, r1 = int(cell_off[c]), int(cell_off[c + 1])
        a0, a1 = int(row_ptr[r0]), int(row_ptr[r1])
        rp = row_ptr[r0:r1 + 1] - row_ptr[r0]
        _lib.check(L.oem_coverage_probs_device(rp.ctypes.data, tid[a0:a1].ctypes.data, s[a0:a1].ctypes.data,
                                               e[a0:a1].ctypes.data, tl.ctypes.data, r1 - r0, a1 - a0, len(tl), 100, 1,
                                               2.0, 0, out[a0:a1].ctypes.data))


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "cells_coverage_bench.json")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    threads = min(16, os.cpu_count() or 4)
    t = time.perf_counter()
    cell_off, row_ptr, tid, p = synth.make_cells(N_CELLS, READS, T, seed=SEED, threads=threads)
    tl, s, e = synth.make_coordinates(tid, T, seed=SEED, zero_span_frac=0.001, threads=threads)
    gen_s = time.perf_counter() - t
    nnz = len(tid)
    c2 = int(cell_off[2])
    a2 = int(row_ptr[c2])
    small = (cell_off[:3], row_ptr[:c2 + 1], tid[:a2])
    # HIP runtime start-up and every path's first use outside the timed calls
    cov_small = oarfish_amd.cells_coverage_probs(*small, s[:a2], e[:a2], tl)
    if "--batched-only" in args:
        oarfish_amd.cells_coverage_probs(cell_off, row_ptr, tid, s, e, tl)
        print(json.dumps({"batched_only": True, "nnz": nnz}))
        return
    per_cell_loop(*small, s[:a2], e[:a2], tl, np.empty(a2))
    oarfish_amd.em_cells_sparse(*small, p[:a2], cov_small, T, max_iter=5)

    runs = {"batched": [], "loop": [], "em": []}
    loop_out = np.empty(nnz)
    got = None
    for _rep in range(2):   # interleaved: a slow spell of the host hits all three
        t = time.perf_counter()
        got = oarfish_amd.cells_coverage_probs(cell_off, row_ptr, tid, s, e, tl)
        runs["batched"].append(time.perf_counter() - t)
        t = time.perf_counter()
        per_cell_loop(cell_off, row_ptr, tid, s, e, tl, loop_out)
        runs["loop"].append(time.perf_counter() - t)
        t = time.perf_counter()
        res = oarfish_amd.em_cells_sparse(cell_off, row_ptr, tid, p, got, T, max_iter=1000, convergence_thresh=1e-3)
        runs["em"].append(time.perf_counter() - t)
        entries = len(res[1])
        del res

    # batched == loop on every cell (the contract): same NaN positions, values to the atomic-sum noise
    same_nan = bool(np.array_equal(np.isnan(got), np.isnan(loop_out)))
    fin = ~np.isnan(loop_out)
    rel = np.abs(got[fin] - loop_out[fin]) / np.maximum(np.abs(loop_out[fin]), 1e-300)
    best = {k: min(v) for k, v in runs.items()}
    line = {
        "workload": "c5_slice_coverage", "n_cells": N_CELLS, "reads_per_cell": READS, "n_txps": T, "nnz": nnz,
        "model": "binomial", "bin_width": 100,
        "batched_s": round(best["batched"], 4), "loop_s": round(best["loop"], 4), "em_sparse_s": round(best["em"], 4),
        "speedup_vs_loop": round(best["loop"] / best["batched"], 2),
        "coverage_over_em": round(best["batched"] / best["em"], 3),
        "batched_runs_s": [round(x, 4) for x in runs["batched"]], "loop_runs_s": [round(x, 4) for x in runs["loop"]],
        "em_runs_s": [round(x, 4) for x in runs["em"]],
        "batched_alignments_per_s": round(nnz / best["batched"], 1),
        "host_bytes_moved": nnz * (4 + 4 + 4 + 8) + 4 * (len(row_ptr)),
        "em_entries": entries,
        "check_vs_loop": {"cells": N_CELLS, "same_nan": same_nan, "nan": int((~fin).sum()),
                          "max_rel": float(rel.max(initial=0.0)), "median_rel": float(np.median(rel)),
                          "ok": bool(same_nan and rel.max(initial=0.0) <= 2e-6)},
        "generate_s": round(gen_s, 2),
    }
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line), flush=True)
    if not line["check_vs_loop"]["ok"]:
        sys.exit("batched result differs from the per-cell loop")


if __name__ == "__main__":
    main()
