#!/usr/bin/env python3
"""Times a bulk --model-coverage store creation (bulk.rs:103-108 followed by the store the EM runs on) at the shape of
BASELINE configs[2] / [3] (synth.make_store(10 M reads, 200 k transcripts), coordinates from synth.make_coordinates,
logistic model), end to end from host buffers, for weight_coding 0 (f64 weights) and 2 (f32 weights):

  composition  oem_coverage_probs_device (the column to the host), then oem_store_create on that column
  fused        oem_store_create_coverage (DeviceStore.with_coverage): one upload, column and weights stay on the device

Each form is timed twice, alternating in one process (a slow spell of the host hits both), and the faster call is kept.
Both stores then run em_run: same iteration count, counts within 1e-10.  One call of each form runs again with
OEM_VERBOSE=1 and its stage laps are recorded, and the fused call's weights are timed both as k_cov_reads' epilogue
and as a pass of their own (OEM_COV_WEIGHTS_PASS, test-only library).  Writes profiles/store_coverage_bench.json (or
--out PATH) and prints it.

usage: store_coverage_bench.py [--out PATH] [--fused-only]
  --fused-only  generate, warm up, one fused call per weight coding, nothing else (the rocprofv3 trace run)"""
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oarfish_amd import _lib, synth  # noqa: E402
from oarfish_amd.types import DeviceStore  # noqa: E402

N_READS, T = 10_000_000, 200_000


def coverage_column(rp, tid, s, e, tl):
    out = np.empty(len(tid))
    _lib.check(_lib.lib().oem_coverage_probs_device(rp.ctypes.data, tid.ctypes.data, s.ctypes.data, e.ctypes.data,
                                                    tl.ctypes.data, len(rp) - 1, len(tid), len(tl), 100, 0, 2.0, 0,
                                                    out.ctypes.data))
    return out


def composition(a, coding):
    rp, tid, p, s, e, tl = a
    cov = coverage_column(rp, tid, s, e, tl)
    return DeviceStore(rp, tid, p, cov, len(tl), weight_coding=coding)


def fused(a, coding):
    return DeviceStore.with_coverage(*a, weight_coding=coding)


def timed(fn, *args):
    t = time.perf_counter()
    st = fn(*args)
    dt = time.perf_counter() - t
    st.close()
    return dt


def stage_laps(fn, *args):
    """The OEM_VERBOSE=1 stage laps of one call, [(stage, ms)] in order."""
    os.environ["OEM_VERBOSE"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+") as f:
        os.dup2(f.fileno(), 2)
        try:
            t = time.perf_counter()
            st = fn(*args)
            total = time.perf_counter() - t
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["OEM_VERBOSE"]
        st.close()
        f.seek(0)
        laps = [(m.group(1).strip(), float(m.group(2))) for m in re.finditer(r"\[oem\] (.+?)\s+([0-9.]+) ms", f.read())]
    return {"total_ms": round(total * 1e3, 1), "laps_ms": laps}


def main():
    args = sys.argv[1:]
    out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "store_coverage_bench.json")
    threads = min(16, os.cpu_count() or 4)
    t = time.perf_counter()
    st = synth.make_store(N_READS, T, threads=threads)
    tl, s, e = synth.make_coordinates(st.tid, T, threads=threads)
    gen_s = time.perf_counter() - t
    full = (st.row_ptr, st.tid, st.as_prob, s, e, tl)
    r1 = 20_000
    a1 = int(st.row_ptr[r1])
    small = (st.row_ptr[:r1 + 1], st.tid[:a1], st.as_prob[:a1], s[:a1], e[:a1], tl)
    for coding in (0, 2):   # HIP start-up and every path's first use outside the timed calls
        composition(small, coding).close()
        fused(small, coding).close()
    if "--fused-only" in args:
        for coding in (0, 2):
            print(json.dumps({"fused_only": True, "weight_coding": coding, "fused_s": round(timed(fused, full, coding), 4)}))
        return
    line = {"workload": "c3_store_coverage", "n_reads": N_READS, "n_txps": T, "nnz": len(st.tid), "model": "logistic",
            "bin_width": 100, "growth_rate": 2.0, "generate_s": round(gen_s, 2), "codings": {}}
    ok = True
    for coding in (0, 2):
        runs = {"composition": [], "fused": []}
        for _rep in range(2):
            runs["composition"].append(timed(composition, full, coding))
            runs["fused"].append(timed(fused, full, coding))
        best = {k: min(v) for k, v in runs.items()}
        with composition(full, coding) as c:
            want, wi = c.em_run()
        with fused(full, coding) as f:
            got, gi = f.em_run()
        err = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300), initial=0.0))
        same = gi.niter == wi.niter and np.allclose(got, want, rtol=1e-10, atol=1e-10)
        ok &= bool(same)
        line["codings"][str(coding)] = {
            "composition_s": round(best["composition"], 4), "fused_s": round(best["fused"], 4),
            "speedup": round(best["composition"] / best["fused"], 3),
            "runs_s": {k: [round(x, 4) for x in v] for k, v in runs.items()},
            "em_niter": [int(gi.niter), int(wi.niter)], "em_max_rel_diff": err, "em_same": bool(same),
            "stages_composition": stage_laps(composition, full, coding),
            "stages_fused": stage_laps(fused, full, coding),
        }
        print(json.dumps({"weight_coding": coding, **{k: line["codings"][str(coding)][k] for k in
                                                        ("composition_s", "fused_s", "speedup", "em_same")}}), flush=True)
    # the weights: k_cov_reads' epilogue (0, the product path) or a pass of their own (1)
    ab = {}
    with _lib.testing():
        for coding in (0, 2):
            for knob in ("0", "1"):
                os.environ["OEM_COV_WEIGHTS_PASS"] = knob
                fused(small, coding).close()
                ts = [timed(fused, full, coding) for _ in range(2)]
                ab[f"coding{coding}_pass{knob}"] = {"best_s": round(min(ts), 4), "stages": stage_laps(fused, full, coding)}
        del os.environ["OEM_COV_WEIGHTS_PASS"]
    line["weights_kernel_ab"] = ab
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(line) + "\n")
    if not ok:
        sys.exit("fused store differs from the composition")


if __name__ == "__main__":
    main()
