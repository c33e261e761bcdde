#!/usr/bin/env python3
"""Times the `.prob` body (write_function.rs:283-332) at BASELINE configs[1] (1 M reads x 60 k transcripts) and at the
bench store (10 M x 200 k), read names of 36 bytes, display_thresh 1e-6, counts from a short EM run:

  (a) parent path   DeviceStore.assignment_probs + writers.write_out_prob to a file on /dev/shm (at the large shape
                    on the store's first 1 M reads, and so labelled: the writer is an interpreter loop over the reads)
  (b) dense floor   oem_assignment_probs alone: the dense E-step and its read-back
  (c) device text   oem_assignment_text end to end from packed names: upload of the names, kernels, read-back of the
                    text into the result (and, separately, with the copy into a NumPy array and the file write)
  (d) its kernels   measure / scan / emit from HIP events (OEM_TEXT_TIMING, test-only library)

(b) and (c) are the better of two calls, both calls recorded.  The device text of the first 1 M reads is compared with
the parent path's file byte for byte.  Writes profiles/assignment_text_bench.json (or --out PATH) and prints it.

usage: assignment_text_bench.py [--out PATH] [--shapes c2,c3]"""
import ctypes as C
import json
import os
import sys
import tempfile
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oarfish_amd import _lib, synth, writers  # noqa: E402
from oarfish_amd.types import DeviceStore, pack_read_names  # noqa: E402

THRESH = 1e-6
SLICE = 1_000_000
SHM = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def raw_text_call(d, counts, blob, off):
    """oem_assignment_text by itself: the result stays in the library's buffer."""
    L = d._lib
    h = C.c_void_p()
    t = time.perf_counter()
    _lib.check(L.oem_assignment_text(d.handle, counts.ctypes.data, THRESH, blob.ctypes.data, off.ctypes.data, C.byref(h)))
    dt = time.perf_counter() - t
    nb = C.c_uint64(0)
    L.oem_text_result_dims(h, C.byref(nb), None, None)
    L.oem_text_result_destroy(h)
    return dt, int(nb.value)


def shape(name):
    st = synth.make_config(name)
    R = st.n_reads
    names = [f"{i:08x}-0000-4000-8000-{i * 2654435761 % 2 ** 48:012x}" for i in range(R)]   # 36 bytes, uuid-shaped
    blob, off = pack_read_names(names, R)
    rec = {"n_reads": R, "n_txps": st.n_txps, "nnz": int(len(st.tid)), "display_thresh": THRESH, "name_bytes": 36}
    with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, st.n_txps) as d:
        counts, _ = d.em_run(None, 100, 1e-3, 50)
        raw_text_call(d, counts, blob, off)                  # first use outside the timed calls
        d.assignment_probs(counts, THRESH)
        # (b)
        tb = [timed(lambda: d.assignment_probs(counts, THRESH))[0] for _ in range(2)]
        rec["b_dense_probs_s"] = [round(x, 4) for x in tb]
        # (c)
        tc = [raw_text_call(d, counts, blob, off) for _ in range(2)]
        rec["c_device_text_s"] = [round(x[0], 4) for x in tc]
        rec["text_bytes"] = tc[0][1]
        path = os.path.join(SHM, f"oem_text_bench_{os.getpid()}")
        tw, _ = timed(lambda: writers.write_out_prob_device(path, d, counts, (blob, off), [], THRESH))
        rec["c_with_numpy_copy_and_file_s"] = round(tw, 4)
        dev_file = open(path + ".prob", "rb").read()
        os.unlink(path + ".prob")
        # (d)
        with _lib.testing():
            os.environ["OEM_TEXT_TIMING"] = "1"
            try:
                with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, st.n_txps) as dt:
                    ms = (C.c_float * 3)()
                    stages = []
                    for _ in range(2):
                        dt.assignment_text(counts, THRESH, (blob, off))
                        _lib.lib().oem_debug_text_last_timing(ms)
                        stages.append([round(float(x), 3) for x in ms])
            finally:
                del os.environ["OEM_TEXT_TIMING"]
        rec["d_kernel_ms_measure_scan_emit"] = stages
    # (a): its own store on the slice, so that the dense vector and the loop are the slice's
    n = min(SLICE, R)
    a1 = int(st.row_ptr[n])
    with DeviceStore(st.row_ptr[: n + 1], st.tid[:a1], st.as_prob[:a1], None, st.n_txps) as d:
        def parent():
            probs = d.assignment_probs(counts, THRESH)
            return writers.write_out_prob(path, st.row_ptr[: n + 1], st.tid[:a1], probs, names[:n], [], THRESH)
        ta, p = timed(parent)
        host_file = open(p, "rb").read()
        os.unlink(p)
        tcs = [raw_text_call(d, counts, blob[: 36 * n], off[: n + 1])[0] for _ in range(2)]
    rec["a_parent_path_s"] = round(ta, 3)
    rec["a_reads"] = n
    rec["a_label"] = "whole store" if n == R else f"first {n} reads of the store"
    rec["c_device_text_same_reads_s"] = [round(x, 4) for x in tcs]
    host_body, dev_body = host_file[host_file.index(b"\n") + 1:], dev_file[dev_file.index(b"\n") + 1:]
    rec["bytes_equal_on_a_reads"] = host_body == dev_body[:len(host_body)]
    rec["a_over_c_same_reads"] = round(ta / min(tcs), 1)
    rec["c_over_b"] = round(min(rec["c_device_text_s"]) / min(tb), 2)
    rec["e_staged_emit"] = "not built: the lane-per-read emit is the only form"
    return rec


def main():
    args = sys.argv[1:]
    out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "assignment_text_bench.json")
    shapes = args[args.index("--shapes") + 1].split(",") if "--shapes" in args else ["c2", "c3"]
    line = {"workload": "assignment_text", "shapes": {}}
    for name in shapes:
        line["shapes"][name] = shape(name)
        print(json.dumps({name: line["shapes"][name]}), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(line) + "\n")
    bad = [k for k, v in line["shapes"].items() if not v["bytes_equal_on_a_reads"] or min(v["c_device_text_same_reads_s"]) >= v["a_parent_path_s"]]
    if bad:
        sys.exit(f"device text differs from, or is slower than, the parent path on {bad}")


if __name__ == "__main__":
    main()
