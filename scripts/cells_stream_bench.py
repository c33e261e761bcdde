#!/usr/bin/env python
"""The per-cell session against what a per-cell caller could do before it, on the slice behind bench.py's
cells.cells_per_s (625 cells x 50 k reads over 60 k transcripts, synth.make_cells).  Best of two runs each:

  (a) oarfish_amd.CellsStream, 8 pushing threads that each slice their cells out of the generated arrays, for a sweep
      of group_nnz (the library's default is the sweep's best point);
  (b) what integration/oarfish-mi355x.patch does: the same 8 threads calling oem_em_run_cells_sparse(n_cells = 1)
      per cell -- the baseline;
  (c) the one-call form em_cells_sparse on the concatenation -- the bound the session can approach.

(a) and (c) are repeated with the per-cell coverage model.  The result goes to --out as JSON (rewritten after every
measurement); with --verbose-run one more session runs under OEM_VERBOSE=1, whose stage record goes to stderr.
"""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _ab  # noqa: E402,F401  (OEM_AB_DIR: A/B against a snapshot build)
import oarfish_amd  # noqa: E402
from oarfish_amd import _lib, synth  # noqa: E402
from oarfish_amd.em import _take_cells_result  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=625)
    ap.add_argument("--cell-reads", type=int, default=50_000)
    ap.add_argument("--txps", type=int, default=60_000)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--sweep-mi", type=int, nargs="*", default=[8, 16, 32, 64, 128])
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--no-coverage", action="store_true")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--verbose-run", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cells_stream_bench.json"))
    args = ap.parse_args()
    T, n = args.txps, args.cells
    t0 = time.perf_counter()
    cell_off, row_ptr, tid, p = synth.make_cells(n, args.cell_reads, T, threads=16)
    co = cell_off.astype(np.int64)
    ao = row_ptr[co].astype(np.int64)
    print(f"[bench] {n} cells, {len(tid)} alignments generated in {time.perf_counter() - t0:.1f} s", flush=True)
    res = dict(cells=n, cell_reads=args.cell_reads, n_txps=T, alignments=int(len(tid)), pushing_threads=args.threads,
               runs_per_point=args.runs, max_iter=1000, conv_thresh=1e-3)

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    def cell(c, s=None, e=None):
        rp = row_ptr[co[c]:co[c + 1] + 1] - row_ptr[co[c]]
        a = slice(ao[c], ao[c + 1])
        return (rp, tid[a], p[a]) + (() if s is None else (s[a], e[a]))

    def threaded(fn):
        """fn(c) for every cell, cells dealt round-robin to the pushing threads."""
        err = []

        def work(k):
            try:
                for c in range(k, n, args.threads):
                    fn(c)
            except BaseException as ex:   # noqa: BLE001
                err.append(ex)
        th = [threading.Thread(target=work, args=(k,)) for k in range(args.threads)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        if err:
            raise err[0]

    def session(group_nnz, coverage=None, s=None, e=None):
        t0 = time.perf_counter()
        tickets = np.zeros(n, dtype=np.int64)
        with oarfish_amd.CellsStream(T, coverage=coverage, group_nnz=group_nnz) as cs:
            def push(c):
                tickets[cs.push(*cell(c, s, e))] = c
            threaded(push)
            t_push = time.perf_counter() - t0
            got = cs.finish()
            dt = time.perf_counter() - t0
            info = cs.info()
        return dt, dict(info, seconds_pushing=t_push), got, tickets

    def best(fn, what):
        runs, keep = [], None
        for _ in range(args.runs):
            r = fn()
            runs.append(r[0])
            if r[0] <= min(runs):
                keep = r
        print(f"[bench] {what}: {[round(x, 3) for x in runs]} s", flush=True)
        return runs, keep

    def one_call(cov_args=None):
        t0 = time.perf_counter()
        if cov_args is None:
            got = oarfish_amd.em_cells_sparse(cell_off, row_ptr, tid, p, None, T)
        else:
            got = oarfish_amd.em_cells_coverage_sparse(cell_off, row_ptr, tid, p, *cov_args)
        return time.perf_counter() - t0, got

    def differs(got, tickets, want):
        """Largest |difference| of a value between the session's cells and the one-call form's (same columns asserted)."""
        gi, gc, gv, _ = got
        wi, wc, wv, _ = want
        worst = 0.0
        for k in range(n):
            c = int(tickets[k])
            a, b = slice(int(gi[k]), int(gi[k + 1])), slice(int(wi[c]), int(wi[c + 1]))
            assert np.array_equal(gc[a], wc[b]), f"ticket {k} (cell {c}): columns differ"
            if a.stop > a.start:
                worst = max(worst, float(np.max(np.abs(gv[a] - wv[b]) / np.maximum(np.abs(wv[b]), 1e-3))))
        return worst

    # (c) the one-call form
    runs, keep = best(one_call, "(c) one call")
    want = keep[1]
    res["one_call"] = dict(seconds_runs=runs, seconds=min(runs), cells_per_s=n / min(runs))
    save()
    # (a) the session, group_nnz sweep; 0 = the library's default
    res["session_sweep"] = []
    for mi in list(args.sweep_mi) + [0]:
        runs, keep = best(lambda: session(mi << 20), f"(a) session group_nnz = {mi} Mi")
        res["session_sweep"].append(dict(group_nnz_mi=mi, seconds_runs=runs, seconds=min(runs), cells_per_s=n / min(runs),
                                         info=keep[1], max_rel_diff_to_one_call=differs(keep[2], keep[3], want)))
        save()
    # (b) one call per cell from the same threads
    if not args.no_baseline:
        L = _lib.lib()

        def per_cell():
            t0 = time.perf_counter()

            def run(c):
                rp, t, q = cell(c)
                off = np.array([0, len(rp) - 1], dtype=np.uint64)
                r = C.c_void_p()
                _lib.check(L.oem_em_run_cells_sparse(off.ctypes.data, 1, rp.ctypes.data, t.ctypes.data, q.ctypes.data, None,
                                                     len(rp) - 1, len(t), T, 0, 1000, 1e-3, C.byref(r)))
                _take_cells_result(r, 1)
            threaded(run)
            return (time.perf_counter() - t0,)
        runs, _ = best(per_cell, "(b) one call per cell")
        res["per_cell_calls"] = dict(seconds_runs=runs, seconds=min(runs), cells_per_s=n / min(runs))
        save()
    # with the per-cell coverage model
    if not args.no_coverage:
        tl, s, e = synth.make_coordinates(tid, T, threads=16)
        cov = dict(bin_width=100, model="binomial", growth_rate=2.0, txp_len=tl)
        runs, keep = best(lambda: one_call((s, e, tl)), "(c) one call, coverage")
        want = keep[1]
        res["one_call_coverage"] = dict(seconds_runs=runs, seconds=min(runs), cells_per_s=n / min(runs))
        save()
        runs, keep = best(lambda: session(0, cov, s, e), "(a) session, coverage, default group_nnz")
        res["session_coverage"] = dict(group_nnz_mi=0, seconds_runs=runs, seconds=min(runs), cells_per_s=n / min(runs),
                                       info=keep[1], max_rel_diff_to_one_call=differs(keep[2], keep[3], want))
        save()
    if args.verbose_run:
        os.environ["OEM_VERBOSE"] = "1"
        dt, info, _, _ = session(0)
        print(f"[bench] verbose session: {dt:.3f} s {info}", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
