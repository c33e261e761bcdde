#!/usr/bin/env python3
"""Times the bulk records session beside the one call it is an alternative to, in one process on the same records: the
shape and generator of scripts/filter_device_bench.py (synth.make_records of BASELINE configs[2]: 10 M reads, 200 k
transcripts, 10.5 M record groups, 3.35 GB of records), no coverage model.

  one_call   oem_store_create_records (DeviceStore.from_records) end to end: the yardstick, measured here and not taken
             from an earlier run
  session    oem_records_stream_*: 1, 2, 4 and 8 pushing threads (thread t pushes batches t, t + n, ... of the records cut
             at group boundaries) x batch sizes x max_staged_records.  End to end = from the first push to finish
             returning; also the time inside finish, the time pushes were blocked, the batches whose device pass had
             started before finish, and that kept / dims equal the one call's
  extra      one more run of the one call and of the best session under a sampler of the device's used memory (peak over
             the idle level), and one of the best session in the test-only library for k_stream_concat's time by HIP events

Each timed call is warmed up on a slice first and repeated (--repeats, default 2); the JSON keeps every repeat.  Writes
profiles/records_stream_bench.json (or --out PATH) and prints it.

usage: records_stream_bench.py [--out PATH] [--reads N] [--txps T] [--repeats K]"""
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THREADS = (1, 2, 4, 8)
BATCH_GROUPS = (1 << 16, 1 << 18, 1 << 20)
MAX_STAGED = (2 << 20, 8 << 20, 32 << 20)


def spread(ts):
    ts = sorted(ts)
    return {"best_s": round(ts[0], 4), "median_s": round(ts[len(ts) // 2], 4), "worst_s": round(ts[-1], 4),
            "runs_s": [round(t, 4) for t in ts]}


def cut(rec, off, batch_groups):
    """[(records pointer, group_off array rebased to 0, n_groups)] of the batches, cut at group boundaries"""
    out = []
    n = len(off) - 1
    for g in range(0, n, batch_groups):
        m = min(batch_groups, n - g)
        o = (off[g:g + m + 1] - off[g]).astype(np.uint64)
        out.append((rec[int(off[g]):int(off[g + m])], o, m))
    return out


def run_session(filters, tl, batches, n_threads, max_staged):
    """one session: (end to end s, s inside finish, info, store dims, kept)"""
    from oarfish_amd.builder import RecordsStream
    tickets = [None] * len(batches)
    errors = []
    with RecordsStream(filters, tl, max_staged_records=max_staged) as s:
        h, push = s.handle, s._lib.oem_records_stream_push

        def pusher(t):
            tk = C.c_uint64(0)
            for k in range(t, len(batches), n_threads):
                r, o, m = batches[k]
                rc = push(h, r.ctypes.data if len(r) else None, o.ctypes.data, m, C.byref(tk))
                if rc:
                    errors.append(rc)
                    return
                tickets[k] = int(tk.value)
        threads = [threading.Thread(target=pusher, args=(t,)) for t in range(n_threads)]
        t0 = time.perf_counter()
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:
            raise RuntimeError(f"push failed: {errors}")
        t1 = time.perf_counter()
        st, kept, dt = s.finish()
        t2 = time.perf_counter()
        info = s.info()
    dims = (st.n_reads, st.nnz)
    st.close()
    return t2 - t0, t2 - t1, info, dims, kept, tickets


class PeakMemory:
    """samples the device's used memory from a thread: the peak over the level at entry"""

    def __enter__(self):
        import torch
        self._torch, self._stop = torch, False
        free, _ = torch.cuda.mem_get_info()
        self._idle_free = self._min_free = free
        self._t = threading.Thread(target=self._run)
        self._t.start()
        return self

    def _run(self):
        while not self._stop:
            free, _ = self._torch.cuda.mem_get_info()
            self._min_free = min(self._min_free, free)
            time.sleep(0.002)

    def __exit__(self, *exc):
        self._stop = True
        self._t.join()
        self.peak_bytes = int(self._idle_free - self._min_free)


def main():
    args = sys.argv[1:]
    opt = lambda k, dflt: type(dflt)(args[args.index(k) + 1]) if k in args else dflt   # noqa: E731
    repeats = opt("--repeats", 2)
    out_path = opt("--out", os.path.join(ROOT, "profiles", "records_stream_bench.json"))
    n_reads, T = opt("--reads", 10_000_000), opt("--txps", 200_000)
    from oarfish_amd import _lib, synth
    from oarfish_amd.types import DeviceStore
    t = time.perf_counter()
    st = synth.make_store(n_reads, T, threads=min(16, os.cpu_count() or 4))
    sr = synth.make_records(st)
    rec, off, tl, filters = sr.records, sr.group_off, sr.txp_len, sr.filters
    line = {"workload": "c3_records_to_store_session", "n_groups": len(off) - 1, "n_records": len(rec),
            "record_bytes": int(rec.nbytes), "n_reads_kept": st.n_reads, "nnz_kept": st.nnz, "n_txps": T,
            "generate_s": round(time.perf_counter() - t, 1), "repeats": repeats}
    del st
    print(json.dumps(line), flush=True)

    # warm-up on a slice: both paths
    n_small = min(200_000, len(off) - 1)
    small = (rec[:int(off[n_small])], off[:n_small + 1])
    s0, _, _ = DeviceStore.from_records(filters, tl, *small)
    s0.close()
    run_session(filters, tl, cut(*small, 1 << 16), 2, 0)

    ts = []
    for _ in range(repeats):
        t = time.perf_counter()
        one, want_kept, want_dt = DeviceStore.from_records(filters, tl, rec, off)
        ts.append(time.perf_counter() - t)
        want_dims = (one.n_reads, one.nnz)
        one.close()
    line["one_call"] = dict(spread(ts), n_reads=want_dims[0], nnz=want_dims[1])
    print(json.dumps({"one_call": line["one_call"]}), flush=True)

    sessions = []
    for bg in BATCH_GROUPS:
        batches = cut(rec, off, bg)
        for ms in MAX_STAGED:
            for nt in THREADS:
                runs = []
                for _ in range(repeats):
                    e2e, fin, info, dims, kept, tickets = run_session(filters, tl, batches, nt, ms)
                    same = bool(dims == want_dims and (nt > 1 or np.array_equal(kept, want_kept)))   # (one thread: the same order)
                    runs.append((e2e, fin, info, same))
                best = min(runs, key=lambda r: r[0])
                row = {"threads": nt, "batch_groups": bg, "max_staged_records": ms, "batches": len(batches),
                       "end_to_end": spread([r[0] for r in runs]), "finish_s": round(best[1], 4),
                       "blocked_us": best[2]["blocked_us"], "batches_before_finish": best[2]["batches_before_finish"],
                       "host_batches": best[2]["host_batches"], "equals_one_call": all(r[3] for r in runs),
                       "over_one_call": round(best[0] / line["one_call"]["best_s"], 3)}
                sessions.append(row)
                print(json.dumps(row), flush=True)
    line["sessions"] = sessions
    best = min(sessions, key=lambda r: r["end_to_end"]["best_s"])
    best_1 = min((r for r in sessions if r["threads"] == 1), key=lambda r: r["end_to_end"]["best_s"])
    key = lambda r: {k: r[k] for k in ("threads", "batch_groups", "max_staged_records")}   # noqa: E731

    # the extras: peak memory of both, the join kernel of the best session
    batches = cut(rec, off, best["batch_groups"])
    with PeakMemory() as pm_one:
        one, _, _ = DeviceStore.from_records(filters, tl, rec, off)
        store_bytes = one.bytes()[0]
        one.close()
    with PeakMemory() as pm_ses:
        run_session(filters, tl, batches, best["threads"], best["max_staged_records"])
    join_ms = C.c_float(0.0)
    with _lib.testing() as L:
        run_session(filters, tl, cut(*small, 1 << 16), 1, 0)
        e2e_t, fin_t, *_ = run_session(filters, tl, batches, best["threads"], best["max_staged_records"])
        L.oem_debug_records_stream_last_join(C.byref(join_ms))
    line["summary"] = {
        "one_call_s": line["one_call"]["best_s"],
        "best_session": dict(key(best), end_to_end_s=best["end_to_end"]["best_s"], finish_s=best["finish_s"],
                             over_one_call=best["over_one_call"]),
        "best_session_one_thread": dict(key(best_1), end_to_end_s=best_1["end_to_end"]["best_s"], finish_s=best_1["finish_s"],
                                        over_one_call=best_1["over_one_call"]),
        "k_stream_concat_ms": round(float(join_ms.value), 3),
        "finish_s_in_the_join_run": round(fin_t, 4),
        "peak_device_bytes_one_call": pm_one.peak_bytes, "peak_device_bytes_best_session": pm_ses.peak_bytes,
        "store_bytes": store_bytes,
        "all_sessions_equal_the_one_call": all(r["equals_one_call"] for r in sessions)}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
