#!/usr/bin/env python3
"""Times the step before the EM -- alignment records -> resident store -- at the bench shape: synth.make_records of
BASELINE configs[2] (10 M reads, 200 k transcripts, ~80 M kept alignments plus decoys and dropped reads).

  host          oem_builder_add_groups (the oem_builder_add_group loop in C: the only path before the device filter),
                then oem_builder_export + oem_store_create, which completes that path to a store
  device        oem_builder_add_groups_device end to end, and from HIP events (test-only library, OEM_FILTER_TIMING=1)
                the record upload, k_filter_measure, the two scans, k_filter_emit and the fraction of the measure
                kernels' time that overlapped a copy; from the host clock the calling thread's copies of the records
                into pinned staging (a second pass over the records that the PCIe floor does not include)
  records       oem_store_create_records end to end, model -1 and model 0 (logistic)
  copy_rate     the box's pinned host -> device copy rate, for the floor records x 40 B / rate

Every step is a child process under its own `timeout` (the records travel through a file in a temporary directory);
each timed call is warmed up on a slice first and repeated, and the JSON keeps every repeat.  Writes
profiles/filter_device_bench.json (or --out PATH) and prints it.

usage: filter_device_bench.py [--out PATH] [--reads N] [--txps T] [--repeats K]"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_TIMEOUT_S = {"copy_rate": 120, "host": 600, "device": 420, "records": 420}


def spread(ts):
    ts = sorted(ts)
    return {"best_s": round(ts[0], 4), "median_s": round(ts[len(ts) // 2], 4), "worst_s": round(ts[-1], 4),
            "runs_s": [round(t, 4) for t in ts]}


def load(d):
    meta = json.load(open(os.path.join(d, "meta.json")))
    rec = np.load(os.path.join(d, "records.npy"), mmap_mode="r")
    off = np.load(os.path.join(d, "group_off.npy"))
    tl = np.load(os.path.join(d, "txp_len.npy"))
    return meta, np.ascontiguousarray(rec), off, tl


def small(rec, off, n=20_000):
    n = min(n, len(off) - 1)
    return rec[:int(off[n])], off[:n + 1]


def step_copy_rate(d, repeats):
    import torch
    n = 1 << 30
    h = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    g = torch.empty(n, dtype=torch.uint8, device="cuda")
    g.copy_(h, non_blocking=True)
    torch.cuda.synchronize()
    out = []
    for _ in range(max(repeats, 3)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.copy_(h, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        out.append(n / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    return {"pinned_h2d_GBps": [round(x, 2) for x in sorted(out)], "bytes": n}


def step_host(d, repeats):
    from oarfish_amd.builder import StoreBuilder
    from oarfish_amd.types import DeviceStore
    meta, rec, off, tl = load(d)
    with StoreBuilder(meta["filters"], tl) as b:
        b.add_groups(*small(rec, off))
    t_add, t_store = [], []
    for _ in range(repeats):
        with StoreBuilder(meta["filters"], tl) as b:
            t = time.perf_counter()
            b.add_groups(rec, off)
            t_add.append(time.perf_counter() - t)
            t = time.perf_counter()
            rp, tid, p, *_ = b.export()
            with DeviceStore(rp, tid, p, None, len(tl)) as st:
                t_store.append(time.perf_counter() - t)
                dims = (st.n_reads, st.nnz)
    return {"add_groups": spread(t_add), "export_plus_store_create": spread(t_store), "n_reads": dims[0], "nnz": dims[1]}


def step_device(d, repeats):
    import ctypes as C
    from oarfish_amd import _lib
    from oarfish_amd.builder import StoreBuilder
    meta, rec, off, tl = load(d)
    with StoreBuilder(meta["filters"], tl) as b:
        b.add_groups(*small(rec, off), device=0)
    ts = []
    for _ in range(repeats):
        with StoreBuilder(meta["filters"], tl) as b:
            t = time.perf_counter()
            b.add_groups(rec, off, device=0)
            ts.append(time.perf_counter() - t)
            dims = b.dims()
    os.environ["OEM_FILTER_TIMING"] = "1"
    events = []
    with _lib.testing() as L:
        for _ in range(repeats):
            with StoreBuilder(meta["filters"], tl) as b:
                b.add_groups(rec, off, device=0)
                ms = (C.c_float * 6)()
                L.oem_debug_filter_last_timing(ms)
                events.append({"upload_ms": round(ms[0], 2), "k_filter_measure_ms": round(ms[1], 2), "scans_ms": round(ms[2], 2),
                               "k_filter_emit_ms": round(ms[3], 2), "measure_overlapped_by_copy": round(ms[4], 3), "host_staging_copy_ms": round(ms[5], 2)})
    return {"add_groups_device": spread(ts), "events": events, "n_reads": dims[0], "nnz": dims[1]}


def step_records(d, repeats):
    from oarfish_amd.types import DeviceStore
    meta, rec, off, tl = load(d)
    out = {}
    for name, cov in (("model_-1", None), ("model_0", "logistic")):
        st, _, _ = DeviceStore.from_records(meta["filters"], tl, *small(rec, off), coverage=cov)
        st.close()
        ts = []
        for _ in range(repeats):
            t = time.perf_counter()
            st, kept, dt = DeviceStore.from_records(meta["filters"], tl, rec, off, coverage=cov)
            ts.append(time.perf_counter() - t)
            dims = (st.n_reads, st.nnz)
            st.close()
        out[name] = dict(spread(ts), n_reads=dims[0], nnz=dims[1], discard=dt)
    return out


STEPS = {"copy_rate": step_copy_rate, "host": step_host, "device": step_device, "records": step_records}


def main():
    args = sys.argv[1:]
    opt = lambda k, dflt: type(dflt)(args[args.index(k) + 1]) if k in args else dflt   # noqa: E731
    repeats = opt("--repeats", 3)
    if "--step" in args:                                              # a child: one step, its JSON on the last line
        print(json.dumps(STEPS[opt("--step", "")](opt("--dir", ""), repeats)))
        return
    out_path = opt("--out", os.path.join(ROOT, "profiles", "filter_device_bench.json"))
    n_reads, T = opt("--reads", 10_000_000), opt("--txps", 200_000)
    from oarfish_amd import synth
    d = tempfile.mkdtemp(prefix="filter_bench_")
    try:
        t = time.perf_counter()
        st = synth.make_store(n_reads, T, threads=min(16, os.cpu_count() or 4))
        sr = synth.make_records(st)
        np.save(os.path.join(d, "records.npy"), sr.records)
        np.save(os.path.join(d, "group_off.npy"), sr.group_off)
        np.save(os.path.join(d, "txp_len.npy"), sr.txp_len)
        json.dump({"filters": sr.filters}, open(os.path.join(d, "meta.json"), "w"))
        line = {"workload": "c3_records_to_store", "n_groups": len(sr.group_off) - 1, "n_records": len(sr.records),
                "record_bytes": int(sr.records.nbytes), "n_reads_kept": st.n_reads, "nnz_kept": st.nnz, "n_txps": T,
                "generate_s": round(time.perf_counter() - t, 1), "repeats": repeats, "steps": {}}
        del st, sr
        print(json.dumps({k: line[k] for k in ("n_groups", "n_records", "record_bytes", "generate_s")}), flush=True)
        for name in ("copy_rate", "host", "device", "records"):
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[name]), sys.executable, os.path.abspath(__file__), "--step", name,
                   "--dir", d, "--repeats", str(repeats)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:                                     # a fault, a hang or a time limit: nothing more on the GPU
                line["steps"][name] = {"failed_rc": r.returncode, "stderr_tail": r.stderr[-600:]}
                print(json.dumps({name: line["steps"][name]}), flush=True)
                break
            line["steps"][name] = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps({name: line["steps"][name]}), flush=True)
        s = line["steps"]
        if all(k in s and "failed_rc" not in s[k] for k in STEPS):
            rate = float(np.median(s["copy_rate"]["pinned_h2d_GBps"]))
            floor = line["record_bytes"] / (rate * 1e9)
            parent = s["host"]["add_groups"]["best_s"] + s["host"]["export_plus_store_create"]["best_s"]
            ev = s["device"]["events"][len(s["device"]["events"]) // 2]
            line["summary"] = {
                "pinned_h2d_GBps": round(rate, 2), "upload_floor_s": round(floor, 4), "parent_path_s": round(parent, 4),
                "one_call_model_-1_s": s["records"]["model_-1"]["best_s"], "one_call_model_0_s": s["records"]["model_0"]["best_s"],
                "one_call_over_floor": round(s["records"]["model_-1"]["best_s"] / floor, 2),
                "parent_over_one_call": round(parent / s["records"]["model_-1"]["best_s"], 2),
                "upload_events_ms": ev["upload_ms"], "host_staging_copy_ms": ev["host_staging_copy_ms"],
                "kernels_plus_scans_ms": round(ev["k_filter_measure_ms"] + ev["scans_ms"] + ev["k_filter_emit_ms"], 2),
                "kernels_share_of_one_call": round((ev["k_filter_measure_ms"] + ev["scans_ms"] + ev["k_filter_emit_ms"]) * 1e-3 /
                                                   s["records"]["model_-1"]["best_s"], 3)}
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(json.dumps(line) + "\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
