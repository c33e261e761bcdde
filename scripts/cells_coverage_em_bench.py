#!/usr/bin/env python3
"""Times a single-cell --model-coverage run from the built store on (single_cell.rs:117-160) on the 625 x 50 k-read
slice of one GPU of BASELINE configs[4] (60 k transcripts, coordinates from synth.make_coordinates), end to end from
host buffers, each the faster of two calls after a warm-up of every path:

  fused        em_cells_coverage_sparse (oem_em_run_cells_coverage_sparse): coverage and EM in one call, the
               column and the weights stay on the device
  composition  cells_coverage_probs, then em_cells_sparse on the column (the two calls a caller made before);
               its two halves are timed too

The two results are compared cell by cell: identical columns and values within one f32 ulp where the iteration counts
agree, the north star (1e-4) where a cell stopped one iteration apart.  Writes the JSON line to
profiles/cells_coverage_em_bench.json (or the path given with --out) and prints it.

usage: cells_coverage_em_bench.py [--out PATH] [--once] [--fused-only] [--cells N]
  --once        one call of each form after the warm-up, no file written (OEM_VERBOSE=1: the stage breakdown)
  --fused-only  generate, warm up and make one fused call, nothing else (the rocprofv3 trace run)
  --cells N     N cells instead of 625 (5 000: BASELINE configs[4] whole); with it only the fused call is timed"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oarfish_amd  # noqa: E402
from oarfish_amd import synth  # noqa: E402

N_CELLS, READS, T, SEED = 625, 50_000, 60_000, 37


def compare(a, b, cell_off):
    """(cells compared, cells whose iteration counts agree, max f32 ulps there, max north-star error elsewhere)."""
    ai, ac, av, ainf = a
    bi, bc, bv, binf = b
    n = len(cell_off) - 1
    same, max_ulps, max_rel, bad = 0, 0, 0.0, []
    for c in range(n):
        sa, sb = slice(int(ai[c]), int(ai[c + 1])), slice(int(bi[c]), int(bi[c + 1]))
        if ainf[c].niter == binf[c].niter:
            same += 1
            if not np.array_equal(ac[sa], bc[sb]):
                bad.append(c)
                continue
            u = np.abs(av[sa].view(np.int32).astype(np.int64) - bv[sb].view(np.int32).astype(np.int64))
            max_ulps = max(max_ulps, int(u.max(initial=0)))
        else:
            if abs(ainf[c].niter - binf[c].niter) > 1:
                bad.append(c)
                continue
            x = np.zeros(T)
            y = np.zeros(T)
            x[ac[sa]] = av[sa]
            y[bc[sb]] = bv[sb]
            reads = int(cell_off[c + 1] - cell_off[c])
            max_rel = max(max_rel, float(np.abs(x - y).max(initial=0.0)) / max(reads, 1))
    return {"cells": n, "same_niter": same, "max_ulps": max_ulps, "max_err_over_reads_other": max_rel,
            "bad_cells": bad[:10], "ok": not bad and max_ulps <= 1 and max_rel <= 1e-4}


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "cells_coverage_em_bench.json")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    n_cells = int(args[args.index("--cells") + 1]) if "--cells" in args else N_CELLS
    threads = min(16, os.cpu_count() or 4)
    t = time.perf_counter()
    cell_off, row_ptr, tid, p = synth.make_cells(n_cells, READS, T, seed=SEED, threads=threads)
    tl, s, e = synth.make_coordinates(tid, T, seed=SEED, zero_span_frac=0.001, threads=threads)
    gen_s = time.perf_counter() - t
    nnz = len(tid)
    c2 = int(cell_off[2])
    a2 = int(row_ptr[c2])
    small = (cell_off[:3], row_ptr[:c2 + 1], tid[:a2], p[:a2], s[:a2], e[:a2], tl)
    # HIP runtime start-up and every path's first use outside the timed calls
    oarfish_amd.em_cells_coverage_sparse(*small, max_iter=5)
    cov_small = oarfish_amd.cells_coverage_probs(cell_off[:3], row_ptr[:c2 + 1], tid[:a2], s[:a2], e[:a2], tl)
    oarfish_amd.em_cells_sparse(cell_off[:3], row_ptr[:c2 + 1], tid[:a2], p[:a2], cov_small, T, max_iter=5)
    full = (cell_off, row_ptr, tid, p, s, e, tl)
    if "--fused-only" in args or n_cells != N_CELLS:
        t = time.perf_counter()
        res = oarfish_amd.em_cells_coverage_sparse(*full)
        dt = time.perf_counter() - t
        sums = np.add.reduceat(res[2].astype(np.float64), res[0][:-1].astype(np.int64))
        print(json.dumps({"fused_only": True, "n_cells": n_cells, "nnz": nnz, "fused_s": round(dt, 4),
                          "entries": len(res[1]), "min_cell_mass": float(sums.min()), "generate_s": round(gen_s, 2)}))
        return
    runs = {"fused": [], "coverage": [], "em": [], "composition": []}
    fused = comp = None
    for _rep in range(1 if "--once" in args else 2):   # interleaved: a slow spell of the host hits both forms
        fused = comp = None
        t = time.perf_counter()
        fused = oarfish_amd.em_cells_coverage_sparse(*full)
        runs["fused"].append(time.perf_counter() - t)
        t = time.perf_counter()
        cov = oarfish_amd.cells_coverage_probs(cell_off, row_ptr, tid, s, e, tl)
        t1 = time.perf_counter()
        comp = oarfish_amd.em_cells_sparse(cell_off, row_ptr, tid, p, cov, T)
        t2 = time.perf_counter()
        runs["coverage"].append(t1 - t)
        runs["em"].append(t2 - t1)
        runs["composition"].append(t2 - t)
        del cov
    check = compare(fused, comp, cell_off)
    best = {k: min(v) for k, v in runs.items()}
    line = {
        "workload": "c5_slice_coverage_em", "n_cells": N_CELLS, "reads_per_cell": READS, "n_txps": T, "nnz": nnz,
        "model": "binomial", "bin_width": 100, "max_iter": 1000, "conv_thresh": 1e-3,
        "fused_s": round(best["fused"], 4), "composition_s": round(best["composition"], 4),
        "composition_coverage_s": round(best["coverage"], 4), "composition_em_s": round(best["em"], 4),
        "speedup": round(best["composition"] / best["fused"], 3),
        "runs_s": {k: [round(x, 4) for x in v] for k, v in runs.items()},
        "entries": len(fused[1]),
        "check_vs_composition": check,
        "generate_s": round(gen_s, 2),
    }
    print(json.dumps(line), flush=True)
    if "--once" not in args:
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(json.dumps(line) + "\n")
    if not check["ok"]:
        sys.exit("fused result differs from the composition")


if __name__ == "__main__":
    main()
