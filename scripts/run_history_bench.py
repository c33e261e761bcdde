#!/usr/bin/env python3
"""What the per-iteration rel_diff record (OEM_OPT_RUN_HISTORY) costs, measured against a build of the parent commit
(a snapshot directory as scripts/build_variant.sh / OEM_AB_DIR use them).  Processes alternate, as scripts/ab_pass.sh
alternates them: parent, in-tree, parent, in-tree ...  Each process holds ONE store (several stores in one process
share the hardware queues, and which chains of the bootstrap then overlap differs from store to store: a first version
of this script measured that, not the option) and, behind settle passes as bench.py settles, times

  * the loop iteration through oem_time_em_iters (HIP events) and through oem_em_run (wall clock, no early exit),
  * a 32-replicate oem_bootstrap (device-drawn resamples, wall clock).

A parent process takes every figure 2 x inner times; an in-tree process takes it alternately with the option off and on
(K = the iterations of the run) on its one store.  The bar for "unchanged" is the spread (max - min) of the PARENT's
own figures over all its processes; medians and that spread go to profiles/run_history_cost.json.

usage: run_history_bench.py <parent_lib_dir> [c3,c2] [processes per side] [inner reps] [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (one HIP runtime in the process, as the package's loader has it)

from oarfish_amd import synth  # noqa: E402

OPT_RUN_HISTORY = 3
SETTLE_PASSES = 200
ITERS = {"c3": 200, "c2": 1000}
BOOT = dict(n_boot=32, max_iter=100, conv_thresh=1e-3, seed=7)


class RunInfo(C.Structure):
    _fields_ = [("niter", C.c_uint32), ("n_passes", C.c_uint32), ("converged", C.c_uint32), ("reserved", C.c_uint32),
                ("rel_diff", C.c_double)]


def load(path):
    L = C.CDLL(path)
    vp, u64, u32, i32, f64 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_double
    L.oem_last_error.restype = C.c_char_p
    L.oem_store_create.argtypes = [vp, vp, vp, vp, u64, u64, u32, i32, vp, C.POINTER(vp)]
    L.oem_store_destroy.argtypes = [vp]
    L.oem_store_destroy.restype = None
    L.oem_store_set_option.argtypes = [vp, u32, u64]
    L.oem_time_m_step.argtypes = [vp, u32, C.POINTER(C.c_float)]
    L.oem_time_em_iters.argtypes = [vp, u32, C.POINTER(C.c_float)]
    L.oem_em_run.argtypes = [vp, vp, u32, f64, u32, vp, C.POINTER(RunInfo)]
    L.oem_bootstrap.argtypes = [vp, u32, u64, vp, vp, u32, f64, vp, vp]
    return L


class Variant:
    def __init__(self, name, L, st, history):
        self.name, self.L, self.history, self.T = name, L, history, st.n_txps
        self.h = C.c_void_p()
        self.check(L.oem_store_create(st.row_ptr.ctypes.data, st.tid.ctypes.data, st.as_prob.ctypes.data, None,
                                      st.n_reads, st.nnz, st.n_txps, 0, None, C.byref(self.h)))
        self.out = np.zeros(st.n_txps)
        self.boot_out = np.zeros((BOOT["n_boot"], st.n_txps))

    def check(self, rc):
        if rc:
            raise RuntimeError(f"{self.name}: {self.L.oem_last_error().decode()}")

    def record(self, k):
        if self.history is not None:   # (the parent's library does not know the option)
            self.check(self.L.oem_store_set_option(self.h, OPT_RUN_HISTORY, k if self.history else 0))

    def settle(self):
        ms = C.c_float(0)
        self.check(self.L.oem_time_m_step(self.h, SETTLE_PASSES, C.byref(ms)))

    def time_iters(self, n):
        self.record(n)
        ms = C.c_float(0)
        self.check(self.L.oem_time_em_iters(self.h, n, C.byref(ms)))
        return ms.value / n * 1e3                                   # us per iteration

    def em_run(self, n):
        self.record(n)
        info = RunInfo()
        t = time.perf_counter()
        self.check(self.L.oem_em_run(self.h, None, n, -1.0, 0xFFFFFFFF, self.out.ctypes.data, C.byref(info)))
        dt = time.perf_counter() - t
        assert info.niter == n
        return dt / n * 1e6                                          # us per iteration, wall clock

    def bootstrap(self):
        self.record(BOOT["max_iter"])
        t = time.perf_counter()
        self.check(self.L.oem_bootstrap(self.h, BOOT["n_boot"], BOOT["seed"], None, None, BOOT["max_iter"],
                                        BOOT["conv_thresh"], self.boot_out.ctypes.data, None))
        return time.perf_counter() - t                               # seconds

    def close(self):
        self.L.oem_store_destroy(self.h)


def summarise(samples):
    return {"median": statistics.median(samples), "min": min(samples), "max": max(samples),
            "spread": max(samples) - min(samples), "samples": samples}


FIGURES = ("time_em_iters_us", "em_run_us", "bootstrap32_s")


def worker(lib_path, wl, is_parent, inner):
    """one process, one store: {figure: {variant: [samples]}} as a JSON line"""
    cfg = synth.CONFIGS[wl]
    st = synth.make_store(cfg["n_reads"], cfg["n_txps"], cfg["kbar"], threads=max(2, min(16, os.cpu_count() or 8)))
    n = ITERS[wl]
    v = Variant("parent" if is_parent else "tree", load(lib_path), st, None if is_parent else False)
    modes = [("parent", None)] * 2 if is_parent else [("off", False), ("on", True)]
    fns = {"time_em_iters_us": lambda: v.time_iters(n), "em_run_us": lambda: v.em_run(n), "bootstrap32_s": v.bootstrap}
    out = {f: {m: [] for m, _ in modes} for f in FIGURES}
    try:
        for _m, h in modes:                                          # first use of every path, untimed
            v.history = h
            v.settle()
            for f in FIGURES:
                fns[f]()
        for f in FIGURES:
            for r in range(inner):
                for m, h in (modes if r % 2 == 0 else modes[::-1]):
                    v.history = h
                    v.settle()
                    out[f][m].append(fns[f]())
    finally:
        v.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    if sys.argv[1] == "--worker":
        return worker(sys.argv[2], sys.argv[3], sys.argv[4] == "parent", int(sys.argv[5]))
    import subprocess
    parent_dir = sys.argv[1]
    wls = (sys.argv[2] if len(sys.argv) > 2 else "c3,c2").split(",")
    procs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    inner = int(sys.argv[4]) if len(sys.argv) > 4 else 4
    libs = {"parent": os.path.join(os.path.abspath(parent_dir), "liboarfish_em.so"),
            "tree": os.path.join(ROOT, "oarfish_amd", "liboarfish_em.so")}
    out = {"what": "processes alternate between the parent commit's library and the in-tree one, one store each, behind "
                   "%d settle passes; in-tree processes alternate OEM_OPT_RUN_HISTORY off / on on their store; the bar is "
                   "the parent's own spread (max - min) over all its samples" % SETTLE_PASSES,
           "processes_per_side": procs, "inner_reps": inner, "workloads": {}}
    for wl in wls:
        samples = {f: {"parent": [], "off": [], "on": []} for f in FIGURES}
        for p in range(procs):
            for side in ("parent", "tree"):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", libs[side], wl, side, str(inner)],
                                   capture_output=True, text=True, timeout=400)
                if r.returncode != 0:   # a failed process ends the measurement: nothing further is started
                    sys.exit(f"{wl} {side} process {p} failed ({r.returncode}):\n{r.stderr[-2000:]}")
                got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
                for f in FIGURES:
                    for m, xs in got[f].items():
                        samples[f][m] += xs
        res = {}
        for f in FIGURES:
            res[f] = {k: summarise(x) for k, x in samples[f].items()}
            bar = res[f]["parent"]["spread"]
            for k in ("off", "on"):
                res[f][k]["median_minus_parent"] = res[f][k]["median"] - res[f]["parent"]["median"]
                res[f][k]["within_parent_spread"] = abs(res[f][k]["median_minus_parent"]) <= bar
            res[f]["on"]["median_minus_off"] = res[f]["on"]["median"] - res[f]["off"]["median"]
            print(wl, f, {k: round(x["median"], 4) for k, x in res[f].items()}, "parent spread", round(bar, 4), flush=True)
        out["workloads"][wl] = {"iterations": ITERS[wl], "bootstrap": BOOT, "figures": res}
    dst = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "run_history_cost.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", dst)


if __name__ == "__main__":
    main()
