#!/usr/bin/env python
"""Collating cells' records by read name: oem_collate_names against the host sort it replaces, on the slice of
scripts/cells_records_bench.py (625 cells x 50 k reads over 60 k transcripts; synth.make_cells, make_cell_records), the
records of every cell shuffled and named by synth.shuffle_cell_records -- once with UUID names, once with
Illumina-style names.  Per name style:

  (a) the device call, end to end (host clock around oem_collate_names), and one more call through the test-only library
      under OEM_COLLATE_TIMING=1: its rounds, and from HIP events the name uploads, the kernels behind each upload chunk
      and the rounds and the cut after the upload; from the host clock the copies into pinned staging;
  (b) the host walk of oem_collate.h (oem_test_collate_host): std::sort of each cell's record indices with the rule's
      comparator, one cell per thread over --threads CPUs, the way the reference's workers spread cells;
  (c) the PCIe floor: the name bytes over the pinned host-to-device rate measured here.

A warm-up on the first cells, then --runs repeats of (a) and (b), alternating; best and spread.  (a) and (b) must give
the same arrays.  The result goes to --out as JSON (rewritten after every measurement).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oarfish_amd import _lib, synth  # noqa: E402
from scripts.cells_records_bench import pinned_rate_gbs  # noqa: E402


def spread(ts):
    return dict(runs_s=[round(t, 4) for t in ts], best_s=round(min(ts), 4), worst_s=round(max(ts), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=625)
    ap.add_argument("--cell-reads", type=int, default=50_000)
    ap.add_argument("--txps", type=int, default=60_000)
    ap.add_argument("--warm-cells", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--styles", nargs="*", default=["uuid", "illumina"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collate_bench.json"))
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("collate_bench: no HIP device")
    T, n = args.txps, args.cells
    t0 = time.perf_counter()
    cells = synth.make_cells(n, args.cell_reads, T, threads=args.threads)
    cr = synth.make_cell_records(cells, T, threads=args.threads)
    del cells
    n_rec, n_groups = len(cr.records), len(cr.group_off) - 1
    cr.records = cr.records[:0]   # only the groups' sizes are needed here
    print(f"[bench] {n} cells, {n_groups} reads, {n_rec} records generated in {time.perf_counter() - t0:.1f} s", flush=True)
    res = dict(cells=n, cell_reads=args.cell_reads, n_txps=T, groups=n_groups, records=n_rec, runs_per_point=args.runs,
               warm_up_cells=min(args.warm_cells, n), host_threads=args.threads)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    rate = pinned_rate_gbs()
    res["pinned_h2d_gbs"] = round(rate, 2)
    save()
    T_ = _lib.testing_lib()
    for style in args.styles:
        t0 = time.perf_counter()
        _, (blob, off), sec, cro = synth.shuffle_cell_records(cr, style=style, threads=args.threads, with_records=False)
        print(f"[bench] {style}: {len(blob)} name bytes generated in {time.perf_counter() - t0:.1f} s", flush=True)
        r = res[style] = dict(name_bytes=int(len(blob)), bytes_per_name=round(len(blob) / n_rec, 2),
                              pcie_floor_s=round(len(blob) / (rate * 1e9), 4))
        out = {k: (np.empty(n_rec, dtype=np.uint32), np.empty(n_rec + 1, dtype=np.uint64), C.c_uint64(0),
                   np.empty(n + 1, dtype=np.uint64)) for k in ("device", "host")}

        def device(L, nc=n):
            o = out["device"]
            nr = int(cro[nc])
            t0 = time.perf_counter()
            _lib.check(L.oem_collate_names(blob.ctypes.data, off.ctypes.data, sec.ctypes.data, nr, cro.ctypes.data, nc,
                                           _lib.OEM_COLLATE_SORT, 0, o[0].ctypes.data, o[1].ctypes.data, C.byref(o[2]), o[3].ctypes.data))
            return time.perf_counter() - t0

        def host(nc=n):
            o = out["host"]
            nr = int(cro[nc])
            t0 = time.perf_counter()
            rc = T_.oem_test_collate_host(blob.ctypes.data, off.ctypes.data, sec.ctypes.data, nr, cro.ctypes.data, nc,
                                          _lib.OEM_COLLATE_SORT, args.threads, o[0].ctypes.data, o[1].ctypes.data, C.byref(o[2]),
                                          o[3].ctypes.data)
            assert rc == _lib.OEM_OK, T_.oem_last_error()
            return time.perf_counter() - t0

        nw = min(args.warm_cells, n)
        device(_lib.lib(), nw)
        host(nw)
        ta, tb = [], []
        for _ in range(args.runs):
            ta.append(device(_lib.lib()))
            tb.append(host())
        ng = int(out["host"][2].value)
        same = (out["device"][2].value == ng and np.array_equal(out["device"][0], out["host"][0])
                and np.array_equal(out["device"][1][:ng + 1], out["host"][1][:ng + 1]) and np.array_equal(out["device"][3], out["host"][3]))
        r["device_call"], r["host_sort"] = spread(ta), spread(tb)
        r["identical_results"] = bool(same)
        r["n_groups"] = ng
        r["host_over_device"] = round(min(tb) / min(ta), 2)
        r["device_over_pcie_floor"] = round(min(ta) / r["pcie_floor_s"], 2)
        print(f"[bench] {style}: (a) device {r['device_call']}  (b) host {r['host_sort']}  identical {same}", flush=True)
        save()
        os.environ["OEM_COLLATE_TIMING"] = "1"
        dt = device(T_)
        del os.environ["OEM_COLLATE_TIMING"]
        info = (C.c_double * 8)()
        _lib.check(T_.oem_debug_collate_last_call(info))
        r["stages"] = dict(call_s=round(dt, 4), rounds=int(info[0]), rounds_that_sorted=int(info[7]), upload_chunks=int(info[1]),
                           batches=int(info[2]), name_uploads_ms=round(info[3], 2), chunk_kernels_ms=round(info[4], 2),
                           rounds_and_cut_ms=round(info[5], 2), staging_copy_host_ms=round(info[6], 2))
        r["stages"]["staging_copy_share_of_call"] = round(info[6] * 1e-3 / dt, 3)
        print(f"[bench] {style}: stages {r['stages']}", flush=True)
        save()
        del blob, off, sec, out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
