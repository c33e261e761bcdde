#!/usr/bin/env python3
"""Times the `.quant` and `.ambig_info.tsv` files (write_function.rs:104-145) at the bench annotation: the 200 k
transcripts of bench.py's c3 store (10 M reads), counts from an EM run to convergence on it, aux counts from the same
store.  synth gives transcripts no names; they are Ensembl-style here (`ENST00000012345.7`, 17 bytes), lengths 200 ..
9 199.

  (a) parent path   writers.write_output to /dev/shm -- an interpreter loop over the transcripts
  (b) device path   writers.write_output_device end to end (names packed, two device calls, three files written), then
                    oem_quant_text and oem_ambig_text each by itself on packed names (the result stays in the library's
                    buffer), and the packing of the names by itself
  (c) its stages    measure / scan / emit from HIP events (OEM_QUANT_TIMING, test-only library), summed over the chunks
  (d) PCIe floor    names, offsets, lens and counts up and the text down (`.quant`), two u32 columns up and the text down
                    (`.ambig_info.tsv`), at the pinned copy rates measured on this machine

Every timed thing is called once untimed first and then REPEATS times; all repeats are kept (the spread is the
result).  The device files are compared with the parent path's byte for byte.
Writes profiles/quant_text_bench.json (or --out PATH) and prints it.

usage: quant_text_bench.py [--out PATH] [--reads N] [--txps N]"""
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

REPEATS = 5
SHM = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
EXTS = (".meta_info.json", ".quant", ".ambig_info.tsv")


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def repeats(fn, n=REPEATS, digits=5):
    fn()
    return [round(timed(fn)[0], digits) for _ in range(n)]


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


def raw_quant(L, blob, off, lens, counts):
    from oarfish_amd import _lib
    h = C.c_void_p()
    _lib.check(L.oem_quant_text(blob.ctypes.data, off.ctypes.data, lens.ctypes.data, counts.ctypes.data, len(lens), None, 0, 0, C.byref(h)))
    nb = C.c_uint64(0)
    L.oem_text_result_dims(h, C.byref(nb), None, None)
    L.oem_text_result_destroy(h)
    return int(nb.value)


def raw_ambig(L, unique, total):
    from oarfish_amd import _lib
    h = C.c_void_p()
    _lib.check(L.oem_ambig_text(unique.ctypes.data, total.ctypes.data, len(unique), None, 0, 0, C.byref(h)))
    nb = C.c_uint64(0)
    L.oem_text_result_dims(h, C.byref(nb), None, None)
    L.oem_text_result_destroy(h)
    return int(nb.value)


def stage_ms(call):
    """measure / scan / emit of REPEATS calls in the test-only library under OEM_QUANT_TIMING."""
    from oarfish_amd import _lib
    os.environ["OEM_QUANT_TIMING"] = "1"
    try:
        with _lib.testing():
            L = _lib.lib()
            out = (C.c_double * 6)()
            call(L)
            rows = []
            for _ in range(REPEATS):
                call(L)
                L.oem_debug_quant_last_call(out)
                rows.append([round(float(x), 4) for x in out[3:6]])
    finally:
        del os.environ["OEM_QUANT_TIMING"]
    return rows


def main():
    args = sys.argv[1:]
    if "--copy-rates" in args:
        print(json.dumps(copy_rates()))
        return
    out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "quant_text_bench.json")
    n_reads = int(args[args.index("--reads") + 1]) if "--reads" in args else 10_000_000
    n_txps = int(args[args.index("--txps") + 1]) if "--txps" in args else 200_000
    # (a process of its own: the copy-rate measurement brings its own runtime)
    rates = json.loads(subprocess.check_output([sys.executable, os.path.abspath(__file__), "--copy-rates"], text=True).splitlines()[-1])

    import oarfish_amd
    from oarfish_amd import _lib, synth, writers
    from oarfish_amd.em import em

    st = synth.make_store(n_reads, n_txps, 8.0, threads=16)
    store = oarfish_amd.InMemoryAlignmentStore.from_arrays(st.row_ptr, st.tid, st.as_prob)
    emi = oarfish_amd.EMInfo(eq_map=store, txp_info=[oarfish_amd.TranscriptInfo()] * n_txps, max_iter=1000, convergence_thresh=1e-3)
    em(emi, 1)
    t_em = repeats(lambda: em(emi, 1), 3, 4)
    counts = em(emi, 1)
    unique, total = store.device_store(n_txps, 0).aux_counts()
    names = [f"ENST{i:011d}.{i % 13}" for i in range(n_txps)]
    lens = (200 + np.arange(n_txps) * 37 % 9000).astype(np.uint64)
    lens_list = lens.tolist()
    rec = {"workload": "quant_text", "n_reads": n_reads, "n_txps": n_txps, "em_iterations": emi.last_run_info.niter,
           "em_converged": bool(emi.last_run_info.converged), "em_call_s": t_em, "repeats": REPEATS, "copy_rates": rates,
           "counts_zero_share": round(float(np.mean(counts == 0.0)), 4)}
    base = os.path.join(SHM, f"oem_quant_bench_{os.getpid()}")
    L = _lib.lib()
    blob, off = writers.pack_names(names)

    # (b)
    rec["b_write_output_device_s"] = repeats(lambda: writers.write_output_device(base + "_dev", {}, names, lens, counts, (unique, total)))
    rec["b_pack_names_s"] = repeats(lambda: writers.pack_names(names))
    rec["b_oem_quant_text_s"] = repeats(lambda: raw_quant(L, blob, off, lens, counts))
    rec["b_oem_ambig_text_s"] = repeats(lambda: raw_ambig(L, unique, total))
    rec["quant_text_bytes"] = raw_quant(L, blob, off, lens, counts)
    rec["ambig_text_bytes"] = raw_ambig(L, unique, total)
    rec["quant_bytes_per_line"] = round(rec["quant_text_bytes"] / n_txps, 2)
    # (c)
    rec["c_quant_kernel_ms_measure_scan_emit"] = stage_ms(lambda Lt: raw_quant(Lt, blob, off, lens, counts))
    rec["c_ambig_kernel_ms_measure_scan_emit"] = stage_ms(lambda Lt: raw_ambig(Lt, unique, total))
    # (d)
    up, down = float(np.median(rates["pinned_h2d_GBps"])), float(np.median(rates["pinned_d2h_GBps"]))
    q_up = len(blob) + 8 * (n_txps + 1) + 16 * n_txps
    rec["quant_bytes_up"] = q_up
    rec["d_quant_pcie_floor_s"] = round(q_up / (up * 1e9) + rec["quant_text_bytes"] / (down * 1e9), 6)
    rec["d_ambig_pcie_floor_s"] = round(8 * n_txps / (up * 1e9) + rec["ambig_text_bytes"] / (down * 1e9), 6)
    # (a)
    rec["a_write_output_s"] = repeats(lambda: writers.write_output(base + "_host", {}, names, lens_list, counts, unique, total))
    rec["files_equal"] = all(open(base + "_host" + e, "rb").read() == open(base + "_dev" + e, "rb").read() for e in EXTS)
    rec["speedup_median"] = round(float(np.median(rec["a_write_output_s"]) / np.median(rec["b_write_output_device_s"])), 2)
    for side in ("_host", "_dev"):
        for e in EXTS:
            os.unlink(base + side + e)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(rec) + "\n")
    if not rec["files_equal"]:
        sys.exit("the device files differ from the parent path's")


if __name__ == "__main__":
    main()
