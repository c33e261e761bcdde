#!/usr/bin/env python3
"""Times projected (genome-mode) records -> resident store at the shape of scripts/filter_device_bench.py:
synth.make_projected_records of BASELINE configs[2] (10 M reads, 200 k transcripts, ~80 M kept alignments plus decoys and
dropped reads), for each probability source (similarity, score, combined).

  one_call      oem_store_create_projected_records end to end, model -1 and model 0 (logistic)
  long_way      the comparison on the same commit: oem_builder_add_projected_groups (the host loop), then
                oem_builder_store_create (model -1) or oem_builder_store_create_coverage (model 0)
  events        oem_builder_add_projected_groups_device under OEM_FILTER_TIMING=1 (test-only library): k_proj_measure
                and k_proj_emit from HIP events, and -- the part filter() does not have -- the alignments whose expf
                the host finished, with the time of that round trip (select, copy down, libm expf, copy up, scatter)

Every step is a child process under its own `timeout` (the records travel through a file in a temporary directory);
each timed call is warmed up on a slice first and repeated, and the JSON keeps every repeat.  Writes
profiles/projected_filter_bench.json (or --out PATH) and prints it.

usage: projected_filter_bench.py [--out PATH] [--reads N] [--txps T] [--repeats K]"""
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

SOURCES = ("similarity", "score", "combined")
STEP_TIMEOUT_S = {"one_call": 420, "long_way": 600, "events": 420}


def spread(ts):
    ts = sorted(ts)
    return {"best_s": round(ts[0], 4), "median_s": round(ts[len(ts) // 2], 4), "worst_s": round(ts[-1], 4),
            "runs_s": [round(t, 4) for t in ts]}


def load(d):
    meta = json.load(open(os.path.join(d, "meta.json")))
    rec = np.ascontiguousarray(np.load(os.path.join(d, "records.npy"), mmap_mode="r"))
    return meta, rec, np.load(os.path.join(d, "group_off.npy")), np.load(os.path.join(d, "read_len.npy")), np.load(os.path.join(d, "txp_len.npy"))


def small(rec, off, rl, n=20_000):
    n = min(n, len(off) - 1)
    return rec[:int(off[n])], off[:n + 1], rl[:n]


def step_one_call(d, repeats):
    from oarfish_amd.types import DeviceStore
    meta, rec, off, rl, tl = load(d)
    out = {}
    for source in SOURCES:
        for name, cov in (("model_-1", None), ("model_0", "logistic")):
            kw = dict(beta=meta["beta"], prob_source=source, coverage=cov)
            DeviceStore.from_projected_records(meta["filters"], tl, *small(rec, off, rl), **kw)[0].close()
            ts = []
            for _ in range(repeats):
                t = time.perf_counter()
                st, kept, dt = DeviceStore.from_projected_records(meta["filters"], tl, rec, off, rl, **kw)
                ts.append(time.perf_counter() - t)
                dims = (st.n_reads, st.nnz)
                st.close()
            out[f"{source}/{name}"] = dict(spread(ts), n_reads=dims[0], nnz=dims[1], discard=dt)
    return out


def step_long_way(d, repeats):
    from oarfish_amd.builder import StoreBuilder
    meta, rec, off, rl, tl = load(d)
    out = {}
    for source in SOURCES:
        kw = dict(beta=meta["beta"], prob_source=source)
        with StoreBuilder(meta["filters"], tl) as b:
            b.add_projected_groups(*small(rec, off, rl), **kw)
            b.device_store().close()
        t_add, t_store = [], {"model_-1": [], "model_0": []}
        for _ in range(repeats):
            with StoreBuilder(meta["filters"], tl) as b:
                t = time.perf_counter()
                b.add_projected_groups(rec, off, rl, **kw)
                t_add.append(time.perf_counter() - t)
                for name, cov in (("model_-1", None), ("model_0", "logistic")):
                    t = time.perf_counter()
                    with b.device_store(coverage=cov) as st:
                        t_store[name].append(time.perf_counter() - t)
                        dims = (st.n_reads, st.nnz)
        out[source] = {"add_projected_groups": spread(t_add), "store_create": spread(t_store["model_-1"]),
                       "store_create_coverage": spread(t_store["model_0"]), "n_reads": dims[0], "nnz": dims[1]}
    return out


def step_events(d, repeats):
    import ctypes as C
    from oarfish_amd import _lib
    from oarfish_amd.builder import StoreBuilder
    meta, rec, off, rl, tl = load(d)
    os.environ["OEM_FILTER_TIMING"] = "1"
    out = {}
    with _lib.testing() as L:
        for source in SOURCES:
            kw = dict(beta=meta["beta"], prob_source=source, device=0)
            with StoreBuilder(meta["filters"], tl) as b:
                b.add_projected_groups(*small(rec, off, rl), **kw)
            runs, ts = [], []
            for _ in range(repeats):
                with StoreBuilder(meta["filters"], tl) as b:
                    t = time.perf_counter()
                    b.add_projected_groups(rec, off, rl, **kw)
                    ts.append(time.perf_counter() - t)
                    v = (C.c_double * 5)()
                    L.oem_debug_proj_last_pass(v)
                    runs.append({"k_proj_measure_ms": round(v[0], 2), "k_proj_emit_ms": round(v[1], 2),
                                 "host_finish_round_trip_ms": round(v[2], 2), "alignments_finished_on_host": int(v[3]),
                                 "alignments_emitted": int(v[4])})
            out[source] = {"add_projected_groups_device": spread(ts), "runs": runs}
    return out


STEPS = {"one_call": step_one_call, "long_way": step_long_way, "events": step_events}


def main():
    args = sys.argv[1:]
    opt = lambda k, dflt: type(dflt)(args[args.index(k) + 1]) if k in args else dflt   # noqa: E731
    repeats = opt("--repeats", 3)
    if "--step" in args:                                              # a child: one step, its JSON on the last line
        print(json.dumps(STEPS[opt("--step", "")](opt("--dir", ""), repeats)))
        return
    out_path = opt("--out", os.path.join(ROOT, "profiles", "projected_filter_bench.json"))
    n_reads, T = opt("--reads", 10_000_000), opt("--txps", 200_000)
    from oarfish_amd import synth
    d = tempfile.mkdtemp(prefix="projected_bench_")
    try:
        t = time.perf_counter()
        st = synth.make_store(n_reads, T, threads=min(16, os.cpu_count() or 4))
        sr = synth.make_projected_records(st)
        for name in ("records", "group_off", "read_len", "txp_len"):
            np.save(os.path.join(d, name + ".npy"), getattr(sr, name))
        json.dump({"filters": sr.filters, "beta": sr.beta}, open(os.path.join(d, "meta.json"), "w"))
        line = {"workload": "c3_projected_records_to_store", "n_groups": len(sr.group_off) - 1, "n_records": len(sr.records),
                "record_bytes": int(sr.records.nbytes), "n_reads_kept": st.n_reads, "nnz_kept": st.nnz, "n_txps": T,
                "beta": sr.beta, "generate_s": round(time.perf_counter() - t, 1), "repeats": repeats, "steps": {}}
        del st, sr
        print(json.dumps({k: line[k] for k in ("n_groups", "n_records", "record_bytes", "generate_s")}), flush=True)
        for name in STEPS:
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
            summary = {}
            for source in SOURCES:
                lw = s["long_way"][source]
                ev = s["events"][source]["runs"][len(s["events"][source]["runs"]) // 2]
                summary[source] = {
                    "one_call_model_-1_s": s["one_call"][f"{source}/model_-1"]["best_s"],
                    "one_call_model_0_s": s["one_call"][f"{source}/model_0"]["best_s"],
                    "long_way_model_-1_s": round(lw["add_projected_groups"]["best_s"] + lw["store_create"]["best_s"], 4),
                    "long_way_model_0_s": round(lw["add_projected_groups"]["best_s"] + lw["store_create_coverage"]["best_s"], 4),
                    "kernels_ms": round(ev["k_proj_measure_ms"] + ev["k_proj_emit_ms"], 2),
                    "alignments_finished_on_host": ev["alignments_finished_on_host"],
                    "host_finish_share_of_alignments": round(ev["alignments_finished_on_host"] / max(1, ev["alignments_emitted"]), 5),
                    "host_finish_round_trip_ms": ev["host_finish_round_trip_ms"]}
            line["summary"] = summary
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(json.dumps(line) + "\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
