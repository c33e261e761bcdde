#!/usr/bin/env python3
"""Times the `.count.mtx` file (write_function.rs:53-54) on two matrices:

  slice   the CSR `em_cells_sparse` returns for the 625-cell x 50 k-read slice of BASELINE configs[4] (60 k transcripts)
  c5      a synthetic CSR of configs[4]'s size: 5 000 cells x 60 k transcripts, 0.18 of them non-zero per cell, values
          log-uniform in (1e-6, 5e4)

  (a) parent path   writers.write_single_cell_output to /dev/shm -- an interpreter loop over the triplets.  On `slice`
                    the whole matrix; on `c5` the first A_CELLS cells only, and so labelled
  (b) device path   writers.write_single_cell_output_device end to end (side files, device text, one write), and
                    oem_count_matrix_text by itself (the result stays in the library's buffer); better of two, both kept
  (c) its stages    measure / scan / emit from HIP events (OEM_MTX_TIMING, test-only library), summed over the chunks
  (d) PCIe floor    8 B up and the text's bytes down per entry, at the pinned copy rates measured on this machine

The device file is compared with the parent path's byte for byte (on `c5`: the lines of the first A_CELLS cells).
Writes profiles/count_matrix_text_bench.json (or --out PATH) and prints it.

usage: count_matrix_text_bench.py [--out PATH] [--shapes slice,c5]"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

A_CELLS = 100
T = 60_000
SHM = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def copy_rates():
    """Pinned host <-> device copy rates (GB/s), from HIP events around 1 GiB copies."""
    import torch
    n = 1 << 30
    h = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    g = torch.empty(n, dtype=torch.uint8, device="cuda")
    out = {}
    for name, (dst, src) in (("pinned_h2d_GBps", (g, h)), ("pinned_d2h_GBps", (h, g))):
        dst.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
        r = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src, non_blocking=True)
            e1.record()
            torch.cuda.synchronize()
            r.append(round(n / (e0.elapsed_time(e1) * 1e-3) / 1e9, 2))
        out[name] = sorted(r)
    return out


def make_slice():
    import oarfish_amd
    from oarfish_amd import synth
    cell_off, row_ptr, tid, p = synth.make_cells(625, 50_000, T, seed=37, threads=16)
    indptr, cols, vals, _ = oarfish_amd.em_cells_sparse(cell_off, row_ptr, tid, p, None, T, max_iter=1000, convergence_thresh=1e-3)
    return indptr, cols, vals


def make_c5():
    rng = np.random.default_rng(505)
    counts, cols = [], []
    for _ in range(10):                                   # 500 cells at a time
        r, c = np.nonzero(rng.random((500, T)) < 0.18)
        counts.append(np.bincount(r, minlength=500))
        cols.append(c.astype(np.uint32))
    cols = np.concatenate(cols)
    indptr = np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.uint64)
    vals = np.exp(rng.uniform(np.log(1e-6), np.log(5e4), len(cols))).astype(np.float32)
    return indptr, cols, vals


def raw_call(L, indptr, cols, vals):
    from oarfish_amd import _lib
    h = C.c_void_p()
    t = time.perf_counter()
    _lib.check(L.oem_count_matrix_text(indptr.ctypes.data, len(indptr) - 1, cols.ctypes.data, vals.ctypes.data, T, 0, None, 0, 0, C.byref(h)))
    dt = time.perf_counter() - t
    nb = C.c_uint64(0)
    L.oem_text_result_dims(h, C.byref(nb), None, None)
    L.oem_text_result_destroy(h)
    return dt, int(nb.value)


def shape(name, rates):
    from oarfish_amd import _lib, writers
    indptr, cols, vals = make_slice() if name == "slice" else make_c5()
    n_cells, nnz = len(indptr) - 1, len(cols)
    rec = {"n_cells": n_cells, "n_txps": T, "entries": nnz, "nonzero_share": round(nnz / (n_cells * T), 4)}
    features = [f"T{i}" for i in range(T)]
    base = os.path.join(SHM, f"oem_mtx_bench_{os.getpid()}")
    L = _lib.lib()
    raw_call(L, indptr[:2], cols[:int(indptr[1])], vals[:int(indptr[1])])             # first use outside the timed calls
    # (b)
    tb = [raw_call(L, indptr, cols, vals) for _ in range(2)]
    rec["b_device_call_s"] = [round(x[0], 4) for x in tb]
    rec["text_bytes"] = tb[0][1]
    rec["bytes_per_line"] = round(tb[0][1] / nnz, 2)
    tw = [timed(lambda: writers.write_single_cell_output_device(base + "_dev", {}, features, None, n_cells, indptr, cols, vals))[0]
          for _ in range(2)]
    rec["b_device_writer_end_to_end_s"] = [round(x, 4) for x in tw]
    # (c)
    os.environ["OEM_MTX_TIMING"] = "1"
    try:
        with _lib.testing():
            ms = (C.c_float * 3)()
            stages = []
            for _ in range(2):
                raw_call(_lib.lib(), indptr, cols, vals)
                _lib.lib().oem_debug_mtx_last_timing(ms)
                stages.append([round(float(x), 3) for x in ms])
    finally:
        del os.environ["OEM_MTX_TIMING"]
    rec["c_kernel_ms_measure_scan_emit"] = stages
    # (d)
    up, down = float(np.median(rates["pinned_h2d_GBps"])), float(np.median(rates["pinned_d2h_GBps"]))
    rec["d_pcie_floor_s"] = round(8 * nnz / (up * 1e9) + tb[0][1] / (down * 1e9), 4)
    # (a)
    a_cells = n_cells if name == "slice" else A_CELLS
    a_nnz = int(indptr[a_cells])
    rows, c, v = writers.csr_triplets(indptr[:a_cells + 1], cols[:a_nnz], vals[:a_nnz])
    ta, _ = timed(lambda: writers.write_single_cell_output(base + "_host", {}, features, None, n_cells, rows, c, v))
    rec["a_parent_path_s"] = round(ta, 3)
    rec["a_entries"] = a_nnz
    rec["a_label"] = "whole matrix" if a_cells == n_cells else f"first {a_cells} of {n_cells} cells"
    rec["a_us_per_entry"] = round(ta / a_nnz * 1e6, 3)
    rec["b_us_per_entry"] = round(min(tw) / nnz * 1e6, 4)
    host, dev = open(base + "_host.count.mtx", "rb").read(), open(base + "_dev.count.mtx", "rb").read()
    # the dimension line counts the entries written: compare what follows it
    def body(data):
        at = 0
        for _ in range(3):
            at = data.index(b"\n", at) + 1
        return data[at:]
    hb = body(host)
    rec["bytes_equal_on_a_entries"] = hb == body(dev)[:len(hb)]
    for side in ("_host", "_dev"):
        for ext in (".count.mtx", ".meta_info.json", ".features.txt"):
            os.unlink(base + side + ext)
    return rec


def main():
    args = sys.argv[1:]
    if "--copy-rates" in args:
        print(json.dumps(copy_rates()))
        return
    out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "count_matrix_text_bench.json")
    shapes = args[args.index("--shapes") + 1].split(",") if "--shapes" in args else ["slice", "c5"]
    # (a process of its own: the copy-rate measurement brings its own runtime)
    rates = json.loads(subprocess.check_output([sys.executable, os.path.abspath(__file__), "--copy-rates"], text=True).splitlines()[-1])
    line = {"workload": "count_matrix_text", "copy_rates": rates, "shapes": {}}
    for name in shapes:
        line["shapes"][name] = shape(name, rates)
        print(json.dumps({name: line["shapes"][name]}), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(line) + "\n")
    bad = [k for k, v in line["shapes"].items() if not v["bytes_equal_on_a_entries"]]
    if bad:
        sys.exit(f"device text differs from the parent path on {bad}")


if __name__ == "__main__":
    main()
