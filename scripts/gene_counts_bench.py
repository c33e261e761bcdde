#!/usr/bin/env python3
"""Times the collapse of the cells x transcripts matrix to cells x genes on the CSR `em_cells_sparse` returns for the
625-cell x 50 k-read slice of BASELINE configs[4] (60 k transcripts), with `synth.gene_of_txps` as the annotation:

  (a) device   em.cells_gene_counts (oem_cells_gene_counts) end to end, from and to host arrays
  (b) host     the NumPy restatement: a stable argsort of the composite key cell * n_genes + gene_of[col], then segment
               sums of the f64 values (np.add.reduceat) rounded to f32

Five repeats each, alternated; best and worst are reported.  One more device call in the test-only library under
OEM_GENE_TIMING=1 gives the split: uploads (with the key kernels behind them) and read-back by the host clock, the sort and
the kernels behind it from HIP events, and the device bytes the call held.  The outputs of (a) and (b) are compared:
offsets and genes exactly; values bit for bit where a run has fewer than eight entries (np.add.reduceat adds pairwise from
eight terms on, the device one after the other), within one f32 ulp elsewhere.

Writes profiles/gene_counts_bench.json (or --out PATH) and prints it.

usage: gene_counts_bench.py [--out PATH] [--cells N]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T = 60_000
REPEATS = 5


def host_gene_counts(indptr, cols, vals, gene_of, n_genes):
    counts = np.diff(indptr.astype(np.int64))
    cell = np.repeat(np.arange(len(counts), dtype=np.uint64), counts)
    key = cell * np.uint64(n_genes) + gene_of[cols].astype(np.uint64)
    order = np.argsort(key, kind="stable")
    key = key[order]
    head = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if len(key) else np.zeros(0, dtype=np.int64)
    sums = np.add.reduceat(vals[order].astype(np.float64), head).astype(np.float32) if len(key) else np.zeros(0, dtype=np.float32)
    heads = key[head]
    genes = (heads % np.uint64(n_genes)).astype(np.uint32)
    indptr_g = np.searchsorted(heads // np.uint64(n_genes), np.arange(len(counts) + 1, dtype=np.uint64)).astype(np.uint64)
    run_len = np.diff(np.concatenate([head, [len(key)]]))
    return (indptr_g, genes, sums), run_len


def main():
    args = sys.argv[1:]
    out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "gene_counts_bench.json")
    n_cells = int(args[args.index("--cells") + 1]) if "--cells" in args else 625
    import oarfish_amd
    from oarfish_amd import _lib, synth
    from oarfish_amd.em import cells_gene_counts
    cell_off, row_ptr, tid, p = synth.make_cells(n_cells, 50_000, T, seed=37, threads=16)
    indptr, cols, vals, _ = oarfish_amd.em_cells_sparse(cell_off, row_ptr, tid, p, None, T, max_iter=1000, convergence_thresh=1e-3)
    gene_of = np.ascontiguousarray(synth.gene_of_txps(T), dtype=np.uint32)
    n_genes = int(gene_of.max()) + 1
    cells_gene_counts(indptr[:2], cols[:int(indptr[1])], vals[:int(indptr[1])], gene_of, n_genes)    # first use outside the timed calls
    ta, tb = [], []
    for _ in range(REPEATS):
        t = time.perf_counter()
        dev = cells_gene_counts(indptr, cols, vals, gene_of, n_genes)
        ta.append(time.perf_counter() - t)
        t = time.perf_counter()
        host, run_len = host_gene_counts(indptr, cols, vals, gene_of, n_genes)
        tb.append(time.perf_counter() - t)
    short = run_len < 8
    ulp = np.abs(dev[2].view(np.int32).astype(np.int64) - host[2].view(np.int32).astype(np.int64))
    equal = bool(np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1]) and len(dev[2]) == len(host[2])
                 and not ulp[short].any() and int(ulp.max(initial=0)) <= 1)
    os.environ["OEM_GENE_TIMING"] = "1"
    try:
        with _lib.testing() as L:
            again = cells_gene_counts(indptr, cols, vals, gene_of, n_genes)
            last = (C.c_double * 6)()
            L.oem_debug_gene_counts_last_call(last)
    finally:
        del os.environ["OEM_GENE_TIMING"]
    equal = equal and all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
                          for a, b in zip(again, dev))
    line = {"workload": "cells_gene_counts", "n_cells": n_cells, "n_txps": T, "n_genes": n_genes, "entries": int(len(cols)),
            "gene_entries": int(len(dev[1])), "longest_run": int(run_len.max(initial=0)), "runs_of_8_or_more": int((run_len >= 8).sum()),
            "a_device_s": {"best": round(min(ta), 4), "worst": round(max(ta), 4), "all": [round(x, 4) for x in ta]},
            "b_host_numpy_s": {"best": round(min(tb), 4), "worst": round(max(tb), 4), "all": [round(x, 4) for x in tb]},
            "split_ms": {"upload_and_keys_host_clock": round(last[0], 3), "sort_hip_events": round(last[1], 3),
                         "heads_scan_sums_cells_hip_events": round(last[2], 3), "read_back_host_clock": round(last[3], 3)},
            "device_bytes": int(last[4]), "batches": int(last[5]), "outputs_equal": equal, "max_ulp_against_host": int(ulp.max(initial=0))}
    print(json.dumps(line))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(line) + "\n")
    if not equal:
        sys.exit("the device result differs from the host restatement")


if __name__ == "__main__":
    main()
