#!/usr/bin/env python
"""Cells from their alignment records in one device call (oem_em_run_cells_records_sparse) against the long way round
on the entry points that existed before it, on the slice behind bench.py's cells.cells_per_s (625 cells x 50 k reads
over 60 k transcripts, synth.make_cells), records from synth.make_cell_records.  Per model (-1: none, 1: binomial):

  (a) the one call, from the records to the entries;
  (b) the long way round, in the same process: a host builder per cell (add_groups over the cell's groups, export,
      discard table), the exports concatenated, then em_cells_sparse / em_cells_coverage_sparse;
  (c) em_cells_sparse (em_cells_coverage_sparse) alone on the exported CSR: what (a) adds in front of the EM is (a) - (c);
  (d) the floor of that excess: the records' bytes at the pinned host-to-device rate measured here.

A warm-up on the first cells, then three repeats of everything, best taken.  One more one-call run goes through the
test-only library under OEM_FILTER_TIMING=1 with one worker: HIP-event times of the filter stages of its last group.
The result goes to --out as JSON (rewritten after every measurement).

--names is a leg of its own (profiles/cells_records_names_bench.json): the same slice as a barcode-collated input holds
it (synth.shuffle_cell_records: every cell's records permuted, each with its read's name), per name style:

  (a) the one call from names and records in input order (oem_em_run_cells_records_names_sparse,
      em_cells_records_sparse(..., names=, collate="device"));
  (b) the path it replaces, by stage: collate_names, the NumPy gather records[order], em_cells_records_sparse;
  (c) em_cells_records_sparse on records that are sorted already: the floor of the filter and EM part.

A warm-up on the first cells, then --runs repeats (default five for this leg) of (a), (b), (c) in turn; best and
spread, (a)/(b), (a) - (c), and the peak of the device memory in use during (a), sampled from another thread.

--barcodes-stream is the leg of the barcoded session (profiles/cells_barcodes_stream_bench.json): the same shuffled, named
slice with a 10x barcode per record, alternated in one process, --runs repeats (five), best to worst:

  (a) the session (CellsStream(barcodes=True), oem_cells_stream_push_barcodes) from one pushing thread, at two batch
      sizes (--batch-records), from the first push to the end of finish;
  (b) the one call on the concatenation (em_cells_records_sparse(..., names=, collate="device"));
  (c) today's session path: CellsStream.push_records(records, names=) per cell -- collate_names, the NumPy gather, the push.

With the peak device memory of (a) and (b) and the session's groups_before_finish.

--umis is the leg of UMI deduplication (profiles/cells_records_umis_bench.json): the --barcodes leg's input (the slice
shuffled, named, with a 10x barcode per record, interleaved uniformly) given UMIs and PCR duplicates by
synth.add_umi_duplicates(rate=0.1), alternated in one process, --runs repeats (five), best to worst:

  (a) the one call with deduplication (oem_em_run_cells_records_umis_sparse, em_cells_records_sparse(..., umis=));
  (b) oem_em_run_cells_records_barcodes_sparse on the same augmented records without UMIs: the duplicates are counted;
  (c) the collate="host" join: collate_barcodes, the NumPy gathers, collate_names, dedup_umis, drop_groups, the records call;
  (d) (a) with every UMI empty.

With (a) - (b), (a)/(c), (d) - (b) beside (b)'s own spread, and the peak device memory of (a) and (b).

--barcodes-any-order-stream is the leg of the any-order barcoded session
(profiles/cells_barcodes_any_order_stream_bench.json): the slice with UUID names and a 10x barcode per record, interleaved
by synth.interleave_cells in both its forms (uniform, blocks), alternated in one process, --runs repeats (five), best to
worst:

  (a) the session (CellsStream(barcodes=True, collated=False)) from one pushing thread at the two --batch-records sizes;
  (b) the one barcodes call on the concatenation (em_cells_records_sparse(..., names=, barcodes=, collate="device")).

With the peak device memory of both, the arena's peak and its bytes per survivor, finish's share of the session's time and
the lookups that missed.  No ratio is promised: the baseline is (b) in the same run.

--umis-rule is the leg of the UMI rule (profiles/cells_records_umis_rule_bench.json): the --umis leg's input with
synth.add_umi_errors(rate=0.05) and a synthetic gene_of, alternated in one process:
  (a) the exact one call; (b) gene keys only; (c) gene keys plus one-mismatch correction; (d) correction without genes.
Reported: (b) - (a) and (c) - (a), the peak device memory, the duplicates and corrected reads per leg, the longest walks of
the neighbour search in both collations and the rounds of pointer jumping.

--umis-stream is the leg of the UMI sessions (profiles/cells_umis_stream_bench.json): the --umis leg's input, alternated
in one process, --runs repeats (five), best to worst, one pushing thread:

  (a) the UMI session (CellsStream(barcodes=True, umis=True)) in both forms at the two --batch-records sizes: the any-order
      form on the input as it is, the collated form on the input ordered stably by each barcode's first record;
  (b) the UMIs one call on the concatenation (em_cells_records_sparse(..., barcodes=, names=, umis=));
  (c) the same sessions without UMIs, which count the duplicates as molecules.

With the peak device memory of each, arena_bytes, the duplicates dropped and (a) - (c).

--whitelist is the leg of barcode correction (profiles/cells_records_whitelist_bench.json): the --umis-rule leg's input
with the cells' barcodes drawn from a 3 M-label whitelist and errors in the barcodes of 5 % of the reads; the whitelist
one call on the raw barcodes against the UMI-rule one call on the clean ones, alternated in one process.

--whitelist-stream is the leg of barcode correction in the any-order session (profiles/cells_whitelist_stream_bench.json):
the --whitelist leg's input cut by synth.cut_interleaved_records at the first --batch-records (2 Mi records), three legs
alternated in one process, five repeats each: (s) the whitelist session on the raw barcodes
(CellsStream(..., collated=False, whitelist=, barcode_multi=True)); (w) the whitelist one call on the concatenation; (c)
the any-order UMI-rule session on the clean barcodes.  Reported: (s) - (c), (s) / (w), the records rejected and deferred,
and the arena's peak.

--umis-rule-stream is the leg of the UMI rule in the sessions (profiles/cells_umis_rule_stream_bench.json): the
--umis-stream leg's input with synth.add_umi_errors(rate=0.05) and a synthetic gene_of, alternated in one process at the
first --batch-records, one pushing thread: both session forms under (a) the exact rule, (b) gene keys, (c) gene keys plus
one-mismatch correction, and the rule one call on the concatenation under (c) beside them.  Reported per form: best to
worst, (b) - (a) and (c) - (a), the duplicates, the corrected reads and the peak device memory.
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

import oarfish_amd  # noqa: E402
from oarfish_amd import _lib, synth  # noqa: E402
from oarfish_amd.builder import StoreBuilder  # noqa: E402

COV = dict(bin_width=100, model="binomial", growth_rate=2.0)


def pinned_rate_gbs(n_bytes=1 << 30, repeats=3):
    """Pinned host-to-device copy rate, GB/s, best of `repeats` (HIP events through torch)."""
    import torch
    h = torch.empty(n_bytes, dtype=torch.uint8, pin_memory=True)
    d = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    d.copy_(h, non_blocking=True)
    torch.cuda.synchronize()
    best = 0.0
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        d.copy_(h, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        best = max(best, n_bytes / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    return best


class PeakDeviceMemory:
    """Samples the device memory in use (hipMemGetInfo through torch) from another thread: the peak above the level at
    entry, in bytes.  The sampling period bounds what it can miss."""

    def __init__(self, period_s=0.002):
        import threading
        import torch
        self._torch, self._period, self._stop = torch, period_s, threading.Event()
        self._thread = threading.Thread(target=self._run, daemon=True)
        self.peak = 0

    def _used(self):
        free, total = self._torch.cuda.mem_get_info()
        return total - free

    def _run(self):
        while not self._stop.is_set():
            self.peak = max(self.peak, self._used() - self._base)
            time.sleep(self._period)

    def __enter__(self):
        self._base = self._used()
        self._thread.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._thread.join()


def spread(ts):
    return dict(runs_s=[round(t, 4) for t in ts], best_s=round(min(ts), 4), worst_s=round(max(ts), 4))


def names_leg(args, cr, res, save):
    """The --names leg (see the module docstring); fills res[style] for every name style."""
    n = args.cells
    f, tl = cr.filters, cr.txp_len

    def clock(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    for style in args.styles:
        t0 = time.perf_counter()
        rec, (blob, off), sec, cro = synth.shuffle_cell_records(cr, style=style, threads=16)
        print(f"[bench] {style}: shuffled and named in {time.perf_counter() - t0:.1f} s ({blob.nbytes / 1e9:.2f} GB of names)", flush=True)
        r = res[style] = dict(name_bytes=int(blob.nbytes), record_bytes=int(rec.nbytes))

        def one_call(nc=n):
            m = int(cro[nc])
            return oarfish_amd.em_cells_records_sparse(f, tl, rec[:m], None, cro[:nc + 1], names=(blob[:int(off[m])], off[:m + 1]),
                                                       secondary=sec[:m], collate="device")

        def two_step(nc=n):
            m = int(cro[nc])
            t_c, (order, goff, cgo) = clock(lambda: oarfish_amd.collate_names((blob[:int(off[m])], off[:m + 1]), cro[:nc + 1], sec[:m]))
            t_g, sorted_rec = clock(lambda: rec[:m][order])
            t_e, got = clock(lambda: oarfish_amd.em_cells_records_sparse(f, tl, sorted_rec, goff, cgo))
            return (t_c, t_g, t_e), got, (sorted_rec, goff, cgo, order)

        nw = min(args.warm_cells, n)
        one_call(nw)
        two_step(nw)
        runs_a, runs_b, runs_c, stages = [], [], [], []
        keep = None
        for k in range(args.runs):
            if k == 0:
                with PeakDeviceMemory() as pk:
                    dt, got_a = clock(one_call)
                r["peak_device_bytes_during_the_call"] = int(pk.peak)
            else:
                dt, got_a = clock(one_call)
            runs_a.append(dt)
            st, got_b, keep = two_step()
            runs_b.append(sum(st))
            stages.append(st)
            runs_c.append(clock(lambda: oarfish_amd.em_cells_records_sparse(f, tl, keep[0], keep[1], keep[2]))[0])
            if k == 0:   # the two paths agree: the exact outputs exactly, the values within an f32 ulp
                assert np.array_equal(got_a[6], keep[3]) and np.array_equal(got_a[4], got_b[4]) and got_a[5] == got_b[5]
                assert np.array_equal(got_a[0], got_b[0]) and np.array_equal(got_a[1], got_b[1])
                ulps = np.abs(got_a[2].view(np.int32).astype(np.int64) - got_b[2].view(np.int32).astype(np.int64))
                r["max_f32_ulps_one_call_to_two_step"] = int(ulps.max(initial=0))
                r["n_groups"] = int(len(keep[1]) - 1)
            del got_a, got_b
            print(f"[bench] {style} run {k}: (a) {runs_a[-1]:.3f} s, (b) {runs_b[-1]:.3f} s = collate {st[0]:.3f} + gather {st[1]:.3f} "
                  f"+ records call {st[2]:.3f}, (c) {runs_c[-1]:.3f} s", flush=True)
            r["one_call"], r["two_step"], r["sorted_records_call"] = spread(runs_a), spread(runs_b), spread(runs_c)
            best = min(range(len(runs_b)), key=lambda i: runs_b[i])
            r["two_step_stages_of_best_run_s"] = dict(collate_names=round(stages[best][0], 4), numpy_gather=round(stages[best][1], 4),
                                                      em_cells_records_sparse=round(stages[best][2], 4))
            r["numpy_gather"] = spread([s[1] for s in stages])
            r["one_call_over_two_step"] = round(min(runs_a) / min(runs_b), 3)
            r["one_call_minus_sorted_records_call_s"] = round(min(runs_a) - min(runs_c), 4)
            save()
        del rec, blob, off, sec, keep


def barcodes_leg(args, cr, res, save):
    """The --barcodes leg: the slice with names, interleaved uniformly, with 10x barcodes.  (a) the one call
    (oem_em_run_cells_records_barcodes_sparse); (b) the collate="host" join by stage -- collate_barcodes, the NumPy gathers
    of records and of names, the names call; (c) oem_em_run_cells_records_names_sparse on the same data already
    barcode-collated.  Also the PCIe floor of barcodes + names + records, the peak device memory and the stage times."""
    import ctypes as C
    from oarfish_amd import _lib
    from oarfish_amd.em import gather_names
    n = args.cells
    f, tl = cr.filters, cr.txp_len
    rate = 57.3   # GB/s pinned, profiles/filter_device_bench.json

    def clock(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    def run(rec, names, sec, bc=None, cro=None, collate="device"):
        if bc is None:
            return oarfish_amd.em_cells_records_sparse(f, tl, rec, None, cro, names=names, secondary=sec, collate="device")
        return oarfish_amd.em_cells_records_sparse(f, tl, rec, None, None, names=names, secondary=sec, barcodes=bc, collate=collate)

    for style in args.styles:
        rec0, names0, sec0, cro = synth.shuffle_cell_records(cr, style=style, threads=16)
        cell_bc = synth.make_barcodes(n, "10x")
        rec, names, sec, bc, _ = synth.interleave_cells(rec0, names0, sec0, cro, cell_bc, how="uniform")
        r = res[style] = dict(name_bytes=int(names[0].nbytes), record_bytes=int(rec.nbytes), barcode_bytes=int(bc[0].nbytes))
        r["pcie_floor_s_at_57.3_gbs"] = round((names[0].nbytes + rec.nbytes + bc[0].nbytes) / (rate * 1e9), 4)
        m = int(cro[min(args.warm_cells, n)])   # warm-up on the first records of the input
        run(rec[:m], (names[0][:int(names[1][m])], names[1][:m + 1]), sec[:m], (bc[0][:int(bc[1][m])], bc[1][:m + 1]))
        runs_a, runs_b, runs_c, stages = [], [], [], []
        for k in range(args.runs):
            os.environ["OEM_COLLATE_TIMING"] = "1" if k == 0 else "0"
            if k == 0:
                with PeakDeviceMemory() as pk:
                    dt, got_a = clock(lambda: run(rec, names, sec, bc))
                r["peak_device_bytes_during_the_call"] = int(pk.peak)
            else:
                dt, got_a = clock(lambda: run(rec, names, sec, bc))
            runs_a.append(dt)
            t_bc, (order_bc, cro_b) = clock(lambda: oarfish_amd.collate_barcodes(bc))
            t_gr, rec_b = clock(lambda: rec[order_bc])
            t_gn, names_b = clock(lambda: gather_names(names, order_bc))
            sec_b = sec[order_bc]
            t_nc, got_b = clock(lambda: run(rec_b, names_b, sec_b, cro=cro_b))
            stages.append((t_bc, t_gr, t_gn, t_nc))
            runs_b.append(sum(stages[-1]))
            runs_c.append(clock(lambda: run(rec_b, names_b, sec_b, cro=cro_b))[0])
            if k == 0:
                assert np.array_equal(got_a[6], order_bc[got_b[6]]) and np.array_equal(got_a[7], cro_b)
                assert np.array_equal(got_a[4], got_b[4]) and got_a[5] == got_b[5]
                assert np.array_equal(got_a[0], got_b[0]) and np.array_equal(got_a[1], got_b[1])
                r["n_cells"] = int(len(cro_b) - 1)
            del got_a, got_b, rec_b, names_b
            print(f"[bench] {style} run {k}: (a) {runs_a[-1]:.3f} s, (b) {runs_b[-1]:.3f} s = barcodes {t_bc:.3f} + records gather {t_gr:.3f} "
                  f"+ names gather {t_gn:.3f} + names call {t_nc:.3f}, (c) {runs_c[-1]:.3f} s", flush=True)
            r["one_call"], r["host_join"], r["names_call_on_collated_input"] = spread(runs_a), spread(runs_b), spread(runs_c)
            best = min(range(len(runs_b)), key=lambda i: runs_b[i])
            r["host_join_stages_of_best_run_s"] = dict(zip(("collate_barcodes", "numpy_gather_records", "numpy_gather_names", "names_call"),
                                                           (round(x, 4) for x in stages[best])))
            r["one_call_over_host_join"] = round(min(runs_a) / min(runs_b), 3)
            r["one_call_minus_names_call_s"] = round(min(runs_a) - min(runs_c), 4)
            save()
        del rec, names, sec, bc, rec0, names0, sec0


def umis_leg(args, cr, res, save):
    """The --umis leg: the --barcodes leg's input (the slice shuffled, named, barcoded, interleaved uniformly) given UMIs
    and PCR duplicates by synth.add_umi_duplicates(rate=0.1).  Alternated in one process: (a) the one call with
    deduplication (oem_em_run_cells_records_umis_sparse); (b) oem_em_run_cells_records_barcodes_sparse on the same
    augmented records without UMIs -- the path that counts the duplicates as molecules; (c) the collate="host" join --
    collate_barcodes, the NumPy gathers, collate_names, dedup_umis, drop_groups, the records call; (d) (a) with every UMI
    empty.  Reported: (a) - (b), the device cost of deduplication (it can be negative: (a) gathers, filters and runs
    fewer reads); (a) / (c); (d) against (b)'s own spread, what an unused UMI argument costs; the peak device memory of
    (a) against (b)."""
    n = args.cells
    f, tl = cr.filters, cr.txp_len

    def clock(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    def run(rec, names, sec, bc, umis=None, collate="device"):
        return oarfish_amd.em_cells_records_sparse(f, tl, rec, None, None, names=names, secondary=sec, barcodes=bc, umis=umis, collate=collate)

    def head(pair, m):
        return pair[0][:int(pair[1][m])], pair[1][:m + 1]

    for style in args.styles:
        rec0, names0, sec0, cro = synth.shuffle_cell_records(cr, style=style, threads=16)
        rec1, names1, sec1, bc1, _ = synth.interleave_cells(rec0, names0, sec0, cro, synth.make_barcodes(n, "10x"), how="uniform")
        del rec0, names0, sec0
        t0 = time.perf_counter()
        rec, names, sec, bc, umis, copies = synth.add_umi_duplicates(rec1, names1, sec1, bc1, rate=0.1)
        r = res[style] = dict(records_before=int(len(rec1)), records=int(len(rec)), copied_reads=int(sum(copies.values())),
                              name_bytes=int(names[0].nbytes), record_bytes=int(rec.nbytes), barcode_bytes=int(bc[0].nbytes),
                              umi_bytes=int(umis[0].nbytes), add_umi_duplicates_s=round(time.perf_counter() - t0, 2))
        del rec1, names1, sec1, bc1
        no_umis = (np.zeros(0, dtype=np.uint8), np.zeros(len(rec) + 1, dtype=np.uint64))
        m = min(len(rec), int(cro[min(args.warm_cells, n)]))   # warm-up on the first records of the input
        for u in (head(umis, m), None):
            run(rec[:m], head(names, m), sec[:m], head(bc, m), u)
        runs = dict(a=[], b=[], c=[], d=[])
        for k in range(args.runs):
            if k == 0:
                with PeakDeviceMemory() as pk:
                    dt, got_a = clock(lambda: run(rec, names, sec, bc, umis))
                r["peak_device_bytes_during_the_one_call"] = int(pk.peak)
            else:
                dt, got_a = clock(lambda: run(rec, names, sec, bc, umis))
            runs["a"].append(dt)
            if k == 0:
                with PeakDeviceMemory() as pk:
                    dt, got_b = clock(lambda: run(rec, names, sec, bc))
                r["peak_device_bytes_during_the_barcodes_call"] = int(pk.peak)
            else:
                dt, got_b = clock(lambda: run(rec, names, sec, bc))
            runs["b"].append(dt)
            dt, got_c = clock(lambda: run(rec, names, sec, bc, umis, collate="host"))
            runs["c"].append(dt)
            runs["d"].append(clock(lambda: run(rec, names, sec, bc, no_umis))[0])
            if k == 0:   # the one call is the join; every copied read is dropped; the barcodes call counts them
                assert all(np.array_equal(got_a[i], got_c[i]) for i in (0, 1, 4, 6, 7, 8)) and got_a[5] == got_c[5]
                assert int(got_a[8].sum()) == sum(copies.values()) and len(got_b[4]) == len(got_a[4]) + int(got_a[8].sum())
                r["n_cells"], r["reads_counted_with_dedup"], r["reads_counted_without"] = int(len(got_a[7]) - 1), int(len(got_a[4])), int(len(got_b[4]))
            del got_a, got_b, got_c
            print(f"[bench] {style} run {k}: (a) {runs['a'][-1]:.3f} s, (b) {runs['b'][-1]:.3f} s, (c) {runs['c'][-1]:.3f} s, (d) {runs['d'][-1]:.3f} s",
                  flush=True)
            r["one_call_with_umis"], r["barcodes_call_without_umis"] = spread(runs["a"]), spread(runs["b"])
            r["host_join"], r["one_call_with_empty_umis"] = spread(runs["c"]), spread(runs["d"])
            r["dedup_device_cost_s_a_minus_b"] = round(min(runs["a"]) - min(runs["b"]), 4)
            r["one_call_over_host_join"] = round(min(runs["a"]) / min(runs["c"]), 3)
            r["empty_umis_minus_barcodes_call_s"] = round(min(runs["d"]) - min(runs["b"]), 4)
            r["barcodes_call_own_spread_s"] = round(max(runs["b"]) - min(runs["b"]), 4)
            save()
        del rec, names, sec, bc, umis


def umis_rule_leg(args, cr, res, save):
    """The --umis-rule leg: the --umis leg's input with sequencing errors in the UMIs (synth.add_umi_errors(rate=0.05), per
    read) and a synthetic annotation (synth.gene_of_txps).  Alternated in one process: (a) the exact one call
    (oem_em_run_cells_records_umis_sparse); (b) gene keys only; (c) gene keys plus one-mismatch correction; (d) correction
    without genes, where a segment is a whole cell.  Reported: (b) - (a) and (c) - (a), the peak device memory, the
    duplicates and the corrected reads per leg, and -- from one more run of (c) and of (d) on the testing library, outside
    the timings -- the classes, the longest neighbour walk in the first and in the halves-swapped collation and the rounds
    of pointer jumping."""
    import ctypes as C
    from oarfish_amd import _lib
    n = args.cells
    f, tl = cr.filters, cr.txp_len

    def clock(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    def head(pair, m):
        return pair[0][:int(pair[1][m])], pair[1][:m + 1]

    for style in args.styles:
        rec0, names0, sec0, cro = synth.shuffle_cell_records(cr, style=style, threads=16)
        rec1, names1, sec1, bc1, _ = synth.interleave_cells(rec0, names0, sec0, cro, synth.make_barcodes(n, "10x"), how="uniform")
        del rec0, names0, sec0
        rec, names, sec, bc, umis, copies = synth.add_umi_duplicates(rec1, names1, sec1, bc1, rate=0.1)
        del rec1, names1, sec1, bc1
        umis = synth.add_umi_errors(umis, 0.05, names=names, barcodes=bc)
        gene_of = synth.gene_of_txps(len(tl))
        r = res[style] = dict(records=int(len(rec)), copied_reads=int(sum(copies.values())), umi_bytes=int(umis[0].nbytes),
                              umi_error_rate=0.05, genes=int(gene_of[-1]) + 1)
        legs = dict(a=dict(), b=dict(gene_of=gene_of), c=dict(gene_of=gene_of, umi_correct=True), d=dict(umi_correct=True))

        def run(kw, upto=None):
            if upto is None:
                return oarfish_amd.em_cells_records_sparse(f, tl, rec, None, None, names=names, secondary=sec, barcodes=bc, umis=umis,
                                                           collate="device", **kw)
            return oarfish_amd.em_cells_records_sparse(f, tl, rec[:upto], None, None, names=head(names, upto), secondary=sec[:upto],
                                                       barcodes=head(bc, upto), umis=head(umis, upto), collate="device", **kw)

        m = min(len(rec), int(cro[min(args.warm_cells, n)]))   # warm-up on the first records of the input
        for kw in legs.values():
            run(kw, m)
        runs = {k: [] for k in legs}
        for k in range(args.runs):
            for leg, kw in legs.items():
                if k == 0:
                    with PeakDeviceMemory() as pk:
                        dt, got = clock(lambda: run(kw))
                    r[f"peak_device_bytes_{leg}"] = int(pk.peak)
                    r[f"duplicates_{leg}"] = int(got[8].sum())
                    r[f"corrected_reads_{leg}"] = int(got[9].sum()) if len(got) > 9 else 0
                    r[f"reads_counted_{leg}"] = int(len(got[4]))
                else:
                    dt, got = clock(lambda: run(kw))
                runs[leg].append(dt)
                del got
            print(f"[bench] {style} run {k}: " + ", ".join(f"({leg}) {runs[leg][-1]:.3f} s" for leg in legs), flush=True)
            r["exact_one_call"], r["gene_keys"] = spread(runs["a"]), spread(runs["b"])
            r["gene_keys_and_correction"], r["correction_without_genes"] = spread(runs["c"]), spread(runs["d"])
            r["gene_keys_cost_s_b_minus_a"] = round(min(runs["b"]) - min(runs["a"]), 4)
            r["gene_keys_and_correction_cost_s_c_minus_a"] = round(min(runs["c"]) - min(runs["a"]), 4)
            r["correction_without_genes_cost_s_d_minus_a"] = round(min(runs["d"]) - min(runs["a"]), 4)
            r["exact_one_call_own_spread_s"] = round(max(runs["a"]) - min(runs["a"]), 4)
            save()
        with _lib.testing() as L:   # what the correction met, from the testing library's counters; not timed
            for leg in ("c", "d"):
                run(legs[leg])
                out = (C.c_double * 8)()
                _lib.check(L.oem_debug_dedup_rule_last_call(out))
                r[f"correction_{leg}"] = dict(participants=int(out[0]), classes=int(out[1]), classes_with_a_parent=int(out[2]),
                                              pointer_jumping_rounds_max=int(out[3]), longest_walk_first_collation=int(out[4]),
                                              longest_walk_swapped_collation=int(out[5]), groups_of_cells=int(out[6]))
        save()
        del rec, names, sec, bc, umis


def whitelist_leg(args, cr, res, save):
    """The --whitelist leg: the --umis-rule leg's input (UMIs with PCR duplicates and errors, a synthetic annotation) with
    the cells' barcodes taken from a whitelist of --whitelist-labels labels (synth.make_whitelist) and sequencing errors in
    the barcodes of 5 % of the reads (synth.add_barcode_errors(rate=0.04, n_rate=0.01), per read).  Alternated in one
    process: (w) the whitelist one call on the RAW barcodes (oem_em_run_cells_records_whitelist_sparse, multi); (c) the
    UMI-rule one call on the same records with the CLEAN barcodes, which is what the parent commit offers to a caller whose
    barcodes were corrected elsewhere.  Both under gene keys plus one-mismatch UMI correction.  Reported: (w) - (c) beside
    (c)'s own spread, the records of every status, the cells, the peak device memory of both."""
    n = args.cells
    f, tl = cr.filters, cr.txp_len

    def clock(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    def head(pair, m):
        return pair[0][:int(pair[1][m])], pair[1][:m + 1]

    t0 = time.perf_counter()
    whitelist = synth.make_whitelist(max(args.whitelist_labels, n))
    labels = [whitelist[0][16 * c:16 * c + 16].tobytes() for c in range(n)]
    res["whitelist_labels"], res["make_whitelist_s"] = int(len(whitelist[1]) - 1), round(time.perf_counter() - t0, 2)
    for style in args.styles:
        rec0, names0, sec0, cro = synth.shuffle_cell_records(cr, style=style, threads=16)
        rec1, names1, sec1, bc1, _ = synth.interleave_cells(rec0, names0, sec0, cro, labels, how="uniform")
        del rec0, names0, sec0
        rec, names, sec, bc, umis, copies = synth.add_umi_duplicates(rec1, names1, sec1, bc1, rate=0.1)
        del rec1, names1, sec1, bc1
        umis = synth.add_umi_errors(umis, 0.05, names=names, barcodes=bc)
        raw = synth.add_barcode_errors(bc, 0.04, 0.01, names=names)
        gene_of = synth.gene_of_txps(len(tl))
        r = res[style] = dict(records=int(len(rec)), copied_reads=int(sum(copies.values())), barcode_bytes=int(bc[0].nbytes),
                              barcode_error_rate=0.05, umi_error_rate=0.05, genes=int(gene_of[-1]) + 1)
        kw = dict(gene_of=gene_of, umi_correct=True, collate="device")

        def run(leg, upto=None):
            b = raw if leg == "w" else bc
            wl = dict(whitelist=whitelist, barcode_multi=True) if leg == "w" else {}
            if upto is None:
                return oarfish_amd.em_cells_records_sparse(f, tl, rec, None, None, names=names, secondary=sec, barcodes=b, umis=umis, **kw, **wl)
            return oarfish_amd.em_cells_records_sparse(f, tl, rec[:upto], None, None, names=head(names, upto), secondary=sec[:upto],
                                                       barcodes=head(b, upto), umis=head(umis, upto), **kw, **wl)

        m = min(len(rec), int(cro[min(args.warm_cells, n)]))   # warm-up on the first records of the input
        for leg in ("w", "c"):
            run(leg, m)
        runs = dict(w=[], c=[])
        for k in range(args.runs):
            for leg in ("w", "c"):
                if k == 0:
                    with PeakDeviceMemory() as pk:
                        dt, got = clock(lambda: run(leg))
                    r[f"peak_device_bytes_{leg}"] = int(pk.peak)
                    r[f"cells_{leg}"], r[f"reads_counted_{leg}"] = int(len(got[7]) - 1), int(len(got[4]))
                    if leg == "w":
                        r["records_by_status"] = dict(zip(("exact", "corrected", "no_neighbour", "ambiguous", "missing"), (int(x) for x in got[12])))
                else:
                    dt, got = clock(lambda: run(leg))
                runs[leg].append(dt)
                del got
            print(f"[bench] {style} run {k}: (w) {runs['w'][-1]:.3f} s, (c) {runs['c'][-1]:.3f} s", flush=True)
            r["whitelist_one_call_on_raw_barcodes"], r["rule_one_call_on_clean_barcodes"] = spread(runs["w"]), spread(runs["c"])
            r["whitelist_cost_s_w_minus_c"] = round(min(runs["w"]) - min(runs["c"]), 4)
            r["clean_call_own_spread_s"] = round(max(runs["c"]) - min(runs["c"]), 4)
            save()
        del rec, names, sec, bc, raw, umis


def whitelist_stream_leg(args, cr, res, save):
    """The --whitelist-stream leg: the --whitelist leg's input (raw barcodes against a whitelist of --whitelist-labels labels,
    UMIs with duplicates and errors, a synthetic annotation) cut by synth.cut_interleaved_records at the first
    --batch-records.  Alternated in one process, from one pushing thread: (s) the whitelist session on the raw barcodes; (w)
    the whitelist one call on the concatenation; (c) the any-order UMI-rule session on the clean barcodes, which is what the
    parent commit offers a streaming caller whose barcodes were corrected elsewhere.  All under gene keys plus one-mismatch
    UMI correction and barcode_multi.  Reported: best - worst of each, (s) - (c) beside (c)'s own spread, (s) / (w), the
    records rejected and deferred, the cells, the arena's peak and the peak device memory of the first run."""
    n = args.cells
    f, tl = cr.filters, cr.txp_len
    batch = args.batch_records[0]

    def clock(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    def head(pair, m):
        return pair[0][:int(pair[1][m])], pair[1][:m + 1]

    whitelist = synth.make_whitelist(max(args.whitelist_labels, n))
    labels = [whitelist[0][16 * c:16 * c + 16].tobytes() for c in range(n)]
    res["whitelist_labels"] = int(len(whitelist[1]) - 1)
    for style in args.styles:
        rec0, names0, sec0, cro = synth.shuffle_cell_records(cr, style=style, threads=16)
        rec1, names1, sec1, bc1, _ = synth.interleave_cells(rec0, names0, sec0, cro, labels, how="uniform")
        del rec0, names0, sec0
        rec, names, sec, bc, umis, copies = synth.add_umi_duplicates(rec1, names1, sec1, bc1, rate=0.1)
        del rec1, names1, sec1, bc1
        umis = synth.add_umi_errors(umis, 0.05, names=names, barcodes=bc)
        raw = synth.add_barcode_errors(bc, 0.04, 0.01, names=names)
        gene_of = synth.gene_of_txps(len(tl))
        m = len(rec)
        r = res[style] = dict(records=int(m), copied_reads=int(sum(copies.values())), barcode_error_rate=0.05, umi_error_rate=0.05,
                              genes=int(gene_of[-1]) + 1, batch_records=int(batch))
        rule = dict(gene_of=gene_of, umi_correct=True)

        def batches(b, upto):
            return synth.cut_interleaved_records(rec[:upto], head(names, upto), sec[:upto], head(b, upto), list(range(batch, upto, batch)),
                                                 umis=head(umis, upto))

        def session(leg, upto=m):
            cut = batches(raw if leg == "s" else bc, upto)   # (views and slices: cut outside the clock)
            wl = dict(whitelist=whitelist, barcode_multi=True) if leg == "s" else {}
            info = {}

            def go():
                with oarfish_amd.CellsStream(len(tl), filters=f, txp_len=tl, barcodes=True, collated=False, umis=True, **rule, **wl) as cs:
                    for records, barcodes, nm, secondary, um in cut:
                        cs.push_batch(records, barcodes, nm, secondary, um)
                    out = cs.finish()
                    cells = cs.cells()
                    info.update(cs.info(), n_cells=len(cells["barcodes"]), reads_counted=int(len(cells["kept"])))
                    if leg == "s":
                        info["counts"] = [int(x) for x in cells["counts"]]
                return out
            dt, out = clock(go)
            return dt, out, info

        def one_call(upto=m):
            return oarfish_amd.em_cells_records_sparse(f, tl, rec[:upto], None, None, names=head(names, upto), secondary=sec[:upto],
                                                       barcodes=head(raw, upto), umis=head(umis, upto), collate="device", whitelist=whitelist,
                                                       barcode_multi=True, **rule)

        warm = min(m, int(cro[min(args.warm_cells, n)]))
        session("s", warm)
        one_call(warm)
        session("c", warm)
        runs = dict(s=[], w=[], c=[])
        for k in range(args.runs):
            for leg in ("s", "w", "c"):
                if leg == "w":
                    if k == 0:
                        with PeakDeviceMemory() as pk:
                            dt, got = clock(one_call)
                        r["peak_device_bytes_w"] = int(pk.peak)
                        r["cells_w"], r["records_by_status_w"] = int(len(got[7]) - 1), [int(x) for x in got[12]]
                    else:
                        dt, got = clock(one_call)
                    del got
                else:
                    if k == 0:
                        with PeakDeviceMemory() as pk:
                            dt, got, info = session(leg)
                        r[f"peak_device_bytes_{leg}"] = int(pk.peak)
                        r[f"cells_{leg}"], r[f"arena_peak_bytes_{leg}"] = info["n_cells"], info["arena_bytes"]
                        if leg == "s":
                            r["records_by_status_s"] = info["counts"]
                            r["barcode_rejected"], r["barcode_deferred"] = info["barcode_rejected"], info["barcode_deferred"]
                    else:
                        dt, got, info = session(leg)
                    del got
                runs[leg].append(dt)
            if k == 0:
                assert r["records_by_status_s"] == r["records_by_status_w"] and r["cells_s"] == r["cells_w"], "the session is not the one call"
            print(f"[bench] {style} run {k}: (s) {runs['s'][-1]:.3f} s, (w) {runs['w'][-1]:.3f} s, (c) {runs['c'][-1]:.3f} s", flush=True)
            r["whitelist_session_on_raw_barcodes"] = spread(runs["s"])
            r["whitelist_one_call_on_raw_barcodes"] = spread(runs["w"])
            r["rule_session_on_clean_barcodes"] = spread(runs["c"])
            r["whitelist_cost_s_s_minus_c"] = round(min(runs["s"]) - min(runs["c"]), 4)
            r["session_over_one_call_s_over_w"] = round(min(runs["s"]) / min(runs["w"]), 3)
            r["clean_session_own_spread_s"] = round(max(runs["c"]) - min(runs["c"]), 4)
            save()
        del rec, names, sec, bc, raw, umis


def barcodes_stream_leg(args, cr, res, save):
    """The --barcodes-stream leg (see the module docstring); fills res[style] for every name style."""
    n = args.cells
    f, tl = cr.filters, cr.txp_len

    def clock(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    for style in args.styles:
        rec, (blob, off), sec, cro = synth.shuffle_cell_records(cr, style=style, threads=16)
        m = len(rec)
        cell_bc = np.frombuffer(b"".join(synth.make_barcodes(n, "10x")), dtype=np.uint8).reshape(n, 18)
        bc_blob = np.repeat(cell_bc, np.diff(cro.astype(np.int64)), axis=0).reshape(-1)   # 18 bytes per record
        r = res[style] = dict(name_bytes=int(blob.nbytes), record_bytes=int(rec.nbytes), barcode_bytes=int(bc_blob.nbytes))

        def session(batch, upto=m):
            info = {}

            def go():
                with oarfish_amd.CellsStream(len(tl), filters=f, txp_len=tl, barcodes=True) as cs:
                    for a in range(0, upto, batch):
                        b = min(a + batch, upto)
                        cs.push_batch(rec[a:b], (bc_blob[18 * a:18 * b], np.arange(b - a + 1, dtype=np.uint64) * 18),
                                      (blob[int(off[a]):int(off[b])], off[a:b + 1] - off[a]), sec[a:b])
                    out = cs.finish()
                    info.update(cs.info(), n_cells=len(cs.cells()["barcodes"]))
                return out
            dt, out = clock(go)
            return dt, out, info

        def one_call(nc=n):
            k = int(cro[nc])
            return oarfish_amd.em_cells_records_sparse(f, tl, rec[:k], None, cro[:nc + 1], names=(blob[:int(off[k])], off[:k + 1]),
                                                       secondary=sec[:k], collate="device")

        def per_cell(nc=n):
            with oarfish_amd.CellsStream(len(tl), filters=f, txp_len=tl) as cs:
                for c in range(nc):
                    a, b = int(cro[c]), int(cro[c + 1])
                    cs.push_records(rec[a:b], names=(blob[int(off[a]):int(off[b])], off[a:b + 1] - off[a]), secondary=sec[a:b])
                return cs.finish()

        nw = min(args.warm_cells, n)
        session(args.batch_records[0], int(cro[nw]))
        one_call(nw)
        per_cell(nw)
        runs_a, runs_b, runs_c = {b: [] for b in args.batch_records}, [], []
        for k in range(args.runs):
            for batch in args.batch_records:
                if k == 0:
                    with PeakDeviceMemory() as pk:
                        dt, got_a, info = session(batch)
                    r[f"session_{batch}_peak_device_bytes"] = int(pk.peak)
                    r[f"session_{batch}_info"] = info
                else:
                    dt, got_a, info = session(batch)
                runs_a[batch].append(dt)
                r[f"session_{batch}_records_per_batch"] = spread(runs_a[batch])
            if k == 0:
                with PeakDeviceMemory() as pk:
                    dt, got_b = clock(one_call)
                r["one_call_peak_device_bytes"] = int(pk.peak)
                assert info["n_cells"] == n and np.array_equal(got_a[0], got_b[0]) and np.array_equal(got_a[1], got_b[1])
                ulps = np.abs(got_a[2].view(np.int32).astype(np.int64) - got_b[2].view(np.int32).astype(np.int64))
                r["max_f32_ulps_session_to_one_call"] = int(ulps.max(initial=0))
            else:
                dt, got_b = clock(one_call)
            runs_b.append(dt)
            del got_a, got_b
            runs_c.append(clock(per_cell)[0])
            r["one_call"], r["push_records_names_per_cell"] = spread(runs_b), spread(runs_c)
            for batch in args.batch_records:
                r[f"session_{batch}_over_one_call"] = round(min(runs_a[batch]) / min(runs_b), 3)
            print(f"[bench] {style} run {k}: (a) " + ", ".join(f"{runs_a[b][-1]:.3f} s at {b}" for b in args.batch_records)
                  + f", (b) {runs_b[-1]:.3f} s, (c) {runs_c[-1]:.3f} s", flush=True)
            save()
        del rec, blob, off, sec, bc_blob


def barcodes_any_order_stream_leg(args, cr, res, save):
    """The --barcodes-any-order-stream leg (see the module docstring); fills res[how] for both interleave_cells forms."""
    from oarfish_amd.em import gather_names
    n = args.cells
    f, tl = cr.filters, cr.txp_len

    def clock(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    rec0, names0, sec0, cro = synth.shuffle_cell_records(cr, style="uuid", threads=16)
    cell_bc = synth.make_barcodes(n, "10x")
    for how in ("uniform", "blocks"):
        rec, (blob, off), sec, (bc_blob, bc_off), _ = synth.interleave_cells(rec0, names0, sec0, cro, cell_bc, how=how)
        off, bc_off = np.asarray(off, dtype=np.uint64), np.asarray(bc_off, dtype=np.uint64)
        m = len(rec)
        r = res[how] = dict(name_bytes=int(blob.nbytes), record_bytes=int(rec.nbytes), barcode_bytes=int(bc_blob.nbytes))
        # the one call's input: the survivors (the session skips the unmapped records and numbers a cell by its first
        # survivor; the one call has no such rule, so it gets what the session keeps)
        S = np.flatnonzero((rec["flags"] & _lib.REC_UNMAPPED) == 0)
        r["records"], r["survivors"] = int(m), int(len(S))
        rec_s, sec_s = rec[S], sec[S]
        names_s, bc_s = gather_names((blob, off), S), gather_names((bc_blob, bc_off), S)

        def session(batch, upto=m):
            info = {}

            def go():
                with oarfish_amd.CellsStream(len(tl), filters=f, txp_len=tl, barcodes=True, collated=False) as cs:
                    for a in range(0, upto, batch):
                        b = min(a + batch, upto)
                        cs.push_batch(rec[a:b], (bc_blob[int(bc_off[a]):int(bc_off[b])], bc_off[a:b + 1] - bc_off[a]),
                                      (blob[int(off[a]):int(off[b])], off[a:b + 1] - off[a]), sec[a:b])
                    t0 = time.perf_counter()
                    out = cs.finish()
                    info.update(cs.info(), finish_s=time.perf_counter() - t0, n_cells=len(cs.cells()["barcodes"]))
                return out
            dt, out = clock(go)
            return dt, out, info

        def one_call(upto=len(S)):
            (nb, no), (bb, bo) = names_s, bc_s
            return oarfish_amd.em_cells_records_sparse(f, tl, rec_s[:upto], None, None, names=(nb[:int(no[upto])], no[:upto + 1]),
                                                       secondary=sec_s[:upto], barcodes=(bb[:int(bo[upto])], bo[:upto + 1]),
                                                       collate="device")

        warm = min(len(S), int(cro[min(args.warm_cells, n)]))
        session(args.batch_records[0], warm)
        one_call(warm)
        runs_a, runs_b, shares = {b: [] for b in args.batch_records}, [], {b: [] for b in args.batch_records}
        for k in range(args.runs):
            for batch in args.batch_records:
                if k == 0:
                    with PeakDeviceMemory() as pk:
                        dt, got_a, info = session(batch)
                    r[f"session_{batch}_peak_device_bytes"] = int(pk.peak)
                    r[f"session_{batch}_info"] = info
                    r[f"session_{batch}_arena_bytes_per_survivor"] = round(info["arena_bytes"] / max(len(S), 1), 2)
                else:
                    dt, got_a, info = session(batch)
                runs_a[batch].append(dt)
                shares[batch].append(info["finish_s"] / dt)
                r[f"session_{batch}_records_per_batch"] = spread(runs_a[batch])
                r[f"session_{batch}_finish_share"] = [round(min(shares[batch]), 3), round(max(shares[batch]), 3)]
            if k == 0:
                with PeakDeviceMemory() as pk:
                    dt, got_b = clock(one_call)
                r["one_call_peak_device_bytes"] = int(pk.peak)
                assert info["n_cells"] == n and np.array_equal(got_a[0], got_b[0]) and np.array_equal(got_a[1], got_b[1])
                ulps = np.abs(got_a[2].view(np.int32).astype(np.int64) - got_b[2].view(np.int32).astype(np.int64))
                r["max_f32_ulps_session_to_one_call"] = int(ulps.max(initial=0))
            else:
                dt, got_b = clock(one_call)
            runs_b.append(dt)
            del got_a, got_b
            r["one_call"] = spread(runs_b)
            for batch in args.batch_records:
                r[f"session_{batch}_over_one_call"] = round(min(runs_a[batch]) / min(runs_b), 3)
            print(f"[bench] {how} run {k}: session " + ", ".join(f"{runs_a[b][-1]:.3f} s at {b}" for b in args.batch_records)
                  + f", one call {runs_b[-1]:.3f} s", flush=True)
            save()
        del rec, blob, off, sec, bc_blob, bc_off, rec_s, sec_s, names_s, bc_s


def umis_stream_leg(args, cr, res, save):
    """The --umis-stream leg: the --umis leg's input (the slice shuffled, named, barcoded, interleaved uniformly, with
    synth.add_umi_duplicates(rate=0.1)).  Alternated in one process, from one pushing thread: (a) the UMI session in both
    forms at every --batch-records -- the any-order form on the input as it is, the collated form on the input ordered
    stably by each barcode's first occurrence; (b) the UMIs one call on the concatenation; (c) the same sessions without
    UMIs, which count the duplicates as molecules.  Reported per form: best - worst of each, peak device memory of the
    first run of each, arena_bytes, the duplicates dropped, and (a) - (c), the cost of the UMIs through the session."""
    from oarfish_amd.em import gather_names
    n = args.cells
    f, tl = cr.filters, cr.txp_len

    def clock(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    for style in args.styles:
        rec0, names0, sec0, cro = synth.shuffle_cell_records(cr, style=style, threads=16)
        rec1, names1, sec1, bc1, _ = synth.interleave_cells(rec0, names0, sec0, cro, synth.make_barcodes(n, "10x"), how="uniform")
        del rec0, names0, sec0
        rec, names, sec, bc, umis, copies = synth.add_umi_duplicates(rec1, names1, sec1, bc1, rate=0.1)
        del rec1, names1, sec1, bc1
        m = len(rec)
        r = res[style] = dict(records=int(m), copied_reads=int(sum(copies.values())), name_bytes=int(names[0].nbytes),
                              record_bytes=int(rec.nbytes), barcode_bytes=int(bc[0].nbytes), umi_bytes=int(umis[0].nbytes))
        order_bc, _ = oarfish_amd.collate_barcodes(bc)          # stable, by each barcode's first record: the collated form's input
        inputs = {"any_order": (rec, names, sec, bc, umis),
                  "collated": (rec[order_bc], gather_names(names, order_bc), sec[order_bc], gather_names(bc, order_bc),
                               gather_names(umis, order_bc))}
        del order_bc

        def session(form, batch, with_umis, upto=m):
            rc, (nb, no), sc, (bb, bo), (ub, uo) = inputs[form]
            no, bo, uo = (np.asarray(o, dtype=np.uint64) for o in (no, bo, uo))
            info = {}

            def go():
                with oarfish_amd.CellsStream(len(tl), filters=f, txp_len=tl, barcodes=True, collated=form == "collated", umis=with_umis) as cs:
                    for a in range(0, upto, batch):
                        b = min(a + batch, upto)
                        u = dict(umis=(ub[int(uo[a]):int(uo[b])], uo[a:b + 1] - uo[a])) if with_umis else {}
                        cs.push_batch(rc[a:b], (bb[int(bo[a]):int(bo[b])], bo[a:b + 1] - bo[a]), (nb[int(no[a]):int(no[b])], no[a:b + 1] - no[a]),
                                      sc[a:b], **u)
                    out = cs.finish()
                    cells = cs.cells()
                    info.update(cs.info(), n_cells=len(cells["barcodes"]), reads=int(len(cells["kept"])))
                return out
            dt, out = clock(go)
            return dt, out, info

        def one_call(upto=m):
            (nb, no), (bb, bo), (ub, uo) = names, bc, umis
            return oarfish_amd.em_cells_records_sparse(f, tl, rec[:upto], None, None, names=(nb[:int(no[upto])], no[:upto + 1]),
                                                       secondary=sec[:upto], barcodes=(bb[:int(bo[upto])], bo[:upto + 1]),
                                                       umis=(ub[:int(uo[upto])], uo[:upto + 1]), collate="device")

        warm = min(m, int(cro[min(args.warm_cells, n)]))
        for form in inputs:
            for with_umis in (True, False):
                session(form, args.batch_records[0], with_umis, warm)
        one_call(warm)
        points = [(form, batch, w) for form in inputs for batch in args.batch_records for w in (True, False)]
        runs, runs_b = {p: [] for p in points}, []
        for k in range(args.runs):
            for p in points:
                form, batch, w = p
                key = f"{form}_{batch}_{'with_umis' if w else 'without_umis'}"
                if k == 0:
                    with PeakDeviceMemory() as pk:
                        dt, got, info = session(*p)
                    r[key + "_peak_device_bytes"] = int(pk.peak)
                    r[key + "_info"] = info
                    if w:   # every copied read is dropped; the record counts add up
                        assert info["umi_dup_reads"] == sum(copies.values()) and info["n_cells"] == n
                else:
                    dt, got, info = session(*p)
                del got
                runs[p].append(dt)
                r[key] = spread(runs[p])
            if k == 0:
                with PeakDeviceMemory() as pk:
                    dt, got_b = clock(one_call)
                r["one_call_peak_device_bytes"] = int(pk.peak)
            else:
                dt, got_b = clock(one_call)
            del got_b
            runs_b.append(dt)
            r["one_call_with_umis"] = spread(runs_b)
            for form in inputs:
                for batch in args.batch_records:
                    a, c = min(runs[(form, batch, True)]), min(runs[(form, batch, False)])
                    r[f"{form}_{batch}_umis_cost_s_a_minus_c"] = round(a - c, 4)
                    r[f"{form}_{batch}_over_one_call"] = round(a / min(runs_b), 3)
            print(f"[bench] {style} run {k}: " + ", ".join(f"{p[0]} {p[1]} {'umis' if p[2] else 'plain'} {runs[p][-1]:.3f} s" for p in points)
                  + f", one call {runs_b[-1]:.3f} s", flush=True)
            save()
        del rec, names, sec, bc, umis, inputs


def umis_rule_stream_leg(args, cr, res, save):
    """The --umis-rule-stream leg: the --umis-stream leg's input with sequencing errors in the UMIs
    (synth.add_umi_errors(rate=0.05)) and a synthetic annotation (synth.gene_of_txps).  Alternated in one process, from one
    pushing thread, at the first --batch-records: both session forms under (a) the exact rule, (b) gene keys, (c) gene keys
    plus correction, and the rule one call on the concatenation under (c) beside them.  Reported per form: best - worst of
    each, (b) - (a) and (c) - (a), the duplicates and the corrected reads, and peak device memory of the first run."""
    from oarfish_amd.em import gather_names
    n = args.cells
    f, tl = cr.filters, cr.txp_len
    batch = args.batch_records[0]

    def clock(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    for style in args.styles:
        rec0, names0, sec0, cro = synth.shuffle_cell_records(cr, style=style, threads=16)
        rec1, names1, sec1, bc1, _ = synth.interleave_cells(rec0, names0, sec0, cro, synth.make_barcodes(n, "10x"), how="uniform")
        del rec0, names0, sec0
        rec, names, sec, bc, umis, copies = synth.add_umi_duplicates(rec1, names1, sec1, bc1, rate=0.1)
        del rec1, names1, sec1, bc1
        umis = synth.add_umi_errors(umis, 0.05, names=names, barcodes=bc)
        gene_of = synth.gene_of_txps(len(tl))
        m = len(rec)
        r = res[style] = dict(records=int(m), copied_reads=int(sum(copies.values())), umi_bytes=int(umis[0].nbytes), umi_error_rate=0.05,
                              genes=int(gene_of[-1]) + 1, batch_records=int(batch))
        order_bc, _ = oarfish_amd.collate_barcodes(bc)
        inputs = {"any_order": (rec, names, sec, bc, umis),
                  "collated": (rec[order_bc], gather_names(names, order_bc), sec[order_bc], gather_names(bc, order_bc),
                               gather_names(umis, order_bc))}
        del order_bc
        rules = dict(a=dict(), b=dict(gene_of=gene_of), c=dict(gene_of=gene_of, umi_correct=True))

        def session(form, rule, upto=m):
            rc, (nb, no), sc, (bb, bo), (ub, uo) = inputs[form]
            no, bo, uo = (np.asarray(o, dtype=np.uint64) for o in (no, bo, uo))
            info = {}

            def go():
                with oarfish_amd.CellsStream(len(tl), filters=f, txp_len=tl, barcodes=True, collated=form == "collated", umis=True,
                                             **rules[rule]) as cs:
                    for a in range(0, upto, batch):
                        b = min(a + batch, upto)
                        cs.push_batch(rc[a:b], (bb[int(bo[a]):int(bo[b])], bo[a:b + 1] - bo[a]), (nb[int(no[a]):int(no[b])], no[a:b + 1] - no[a]),
                                      sc[a:b], umis=(ub[int(uo[a]):int(uo[b])], uo[a:b + 1] - uo[a]))
                    out = cs.finish()
                    info.update(cs.info(), n_cells=len(cs.cells()["barcodes"]))
                return out
            dt, out = clock(go)
            return dt, out, info

        def one_call(upto=m):
            (nb, no), (bb, bo), (ub, uo) = names, bc, umis
            return oarfish_amd.em_cells_records_sparse(f, tl, rec[:upto], None, None, names=(nb[:int(no[upto])], no[:upto + 1]),
                                                       secondary=sec[:upto], barcodes=(bb[:int(bo[upto])], bo[:upto + 1]),
                                                       umis=(ub[:int(uo[upto])], uo[:upto + 1]), collate="device", **rules["c"])

        warm = min(m, int(cro[min(args.warm_cells, n)]))
        for form in inputs:
            for rule in rules:
                session(form, rule, warm)
        one_call(warm)
        points = [(form, rule) for form in inputs for rule in rules]
        runs, runs_one = {p: [] for p in points}, []
        for k in range(args.runs):
            for p in points:
                key = f"{p[0]}_{p[1]}"
                if k == 0:
                    with PeakDeviceMemory() as pk:
                        dt, got, info = session(*p)
                    r[key + "_peak_device_bytes"] = int(pk.peak)
                    r[key + "_duplicates"], r[key + "_corrected_reads"] = info["umi_dup_reads"], info["umi_corrected_reads"]
                else:
                    dt, got, info = session(*p)
                del got
                runs[p].append(dt)
                r[key] = spread(runs[p])
            dt, got = clock(one_call)
            if k == 0:
                r["one_call_c_duplicates"], r["one_call_c_corrected_reads"] = int(got[8].sum()), int(got[9].sum())
                assert r["one_call_c_duplicates"] == r["any_order_c_duplicates"] and r["one_call_c_corrected_reads"] == r["any_order_c_corrected_reads"]
            del got
            runs_one.append(dt)
            r["one_call_c"] = spread(runs_one)
            for form in inputs:
                r[f"{form}_gene_keys_cost_s_b_minus_a"] = round(min(runs[(form, "b")]) - min(runs[(form, "a")]), 4)
                r[f"{form}_gene_keys_and_correction_cost_s_c_minus_a"] = round(min(runs[(form, "c")]) - min(runs[(form, "a")]), 4)
                r[f"{form}_a_own_spread_s"] = round(max(runs[(form, "a")]) - min(runs[(form, "a")]), 4)
            print(f"[bench] {style} run {k}: " + ", ".join(f"{p[0]} ({p[1]}) {runs[p][-1]:.3f} s" for p in points)
                  + f", one call (c) {runs_one[-1]:.3f} s", flush=True)
            save()
        del rec, names, sec, bc, umis, inputs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=625)
    ap.add_argument("--cell-reads", type=int, default=50_000)
    ap.add_argument("--txps", type=int, default=60_000)
    ap.add_argument("--warm-cells", type=int, default=20)
    ap.add_argument("--runs", type=int, default=None, help="repeats per point (3; 5 with --names)")
    ap.add_argument("--models", type=int, nargs="*", default=[-1, 1])
    ap.add_argument("--names", action="store_true", help="the leg from names and records in input order")
    ap.add_argument("--barcodes", action="store_true", help="the leg from records in any order: cells from barcodes")
    ap.add_argument("--umis", action="store_true", help="the leg of the one call with UMI deduplication against the barcodes call and the host join")
    ap.add_argument("--umis-rule", action="store_true",
                    help="the leg of the UMI rule: the exact one call against gene keys, gene keys plus correction, correction alone")
    ap.add_argument("--whitelist", action="store_true",
                    help="the leg of barcode correction: the whitelist one call on raw barcodes against the UMI-rule one call on clean ones")
    ap.add_argument("--whitelist-labels", type=int, default=3_000_000, help="the --whitelist legs: labels of the whitelist")
    ap.add_argument("--whitelist-stream", action="store_true",
                    help="the leg of barcode correction in the any-order session against the whitelist one call and the session on clean barcodes")
    ap.add_argument("--barcodes-stream", action="store_true", help="the leg of the barcoded session against the one call and push_records(names=)")
    ap.add_argument("--barcodes-any-order-stream", action="store_true",
                    help="the leg of the any-order barcoded session against the one barcodes call on the concatenation")
    ap.add_argument("--umis-stream", action="store_true",
                    help="the leg of the UMI sessions (both forms) against the UMIs one call and the sessions without UMIs")
    ap.add_argument("--umis-rule-stream", action="store_true",
                    help="the leg of the UMI rule in the sessions: both forms under the exact rule, gene keys, gene keys plus correction")
    ap.add_argument("--batch-records", type=int, nargs="*", default=[1 << 21, 1 << 23], help="the session legs: records per pushed batch")
    ap.add_argument("--styles", nargs="*", default=["uuid", "illumina"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.runs is None:
        args.runs = 5 if args.names or args.barcodes or args.umis or args.umis_rule or args.whitelist or args.whitelist_stream or args.barcodes_stream or args.barcodes_any_order_stream or args.umis_stream or args.umis_rule_stream else 3
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "cells_whitelist_stream_bench.json" if args.whitelist_stream else
                                "cells_umis_rule_stream_bench.json" if args.umis_rule_stream else
                                "cells_umis_stream_bench.json" if args.umis_stream else
                                "cells_barcodes_any_order_stream_bench.json" if args.barcodes_any_order_stream else
                                "cells_barcodes_stream_bench.json" if args.barcodes_stream else
                                "cells_records_whitelist_bench.json" if args.whitelist else
                                "cells_records_umis_rule_bench.json" if args.umis_rule else
                                "cells_records_umis_bench.json" if args.umis else
                                "cells_records_barcodes_bench.json" if args.barcodes else
                                "cells_records_names_bench.json" if args.names else "cells_records_bench.json")
    T, n = args.txps, args.cells
    t0 = time.perf_counter()
    cells = synth.make_cells(n, args.cell_reads, T, threads=16)
    cr = synth.make_cell_records(cells, T, threads=16)
    del cells
    rec, goff, cgo = cr.records, cr.group_off, cr.cell_group_off
    print(f"[bench] {n} cells, {len(goff) - 1} reads, {len(rec)} records generated in {time.perf_counter() - t0:.1f} s", flush=True)
    res = dict(cells=n, cell_reads=args.cell_reads, n_txps=T, groups=int(len(goff) - 1), records=int(len(rec)),
               record_bytes=int(rec.nbytes), runs_per_point=args.runs, warm_up_cells=min(args.warm_cells, n), max_iter=1000,
               conv_thresh=1e-3)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    def one_call(model, nc=n):
        g1 = int(cgo[nc])
        t0 = time.perf_counter()
        got = oarfish_amd.em_cells_records_sparse(cr.filters, cr.txp_len, rec[:int(goff[g1])], goff[:g1 + 1], cgo[:nc + 1],
                                                  coverage=None if model < 0 else COV)
        return time.perf_counter() - t0, got

    def long_way(model, nc=n):
        """-> (seconds, seconds of the host builders + export + concatenation, result, the exported CSR)"""
        t0 = time.perf_counter()
        co, rps, tids, ps, ss, es, base = np.zeros(nc + 1, dtype=np.uint64), [np.zeros(1, dtype=np.uint64)], [], [], [], [], 0
        tables = []
        for c in range(nc):
            g0, g1 = int(cgo[c]), int(cgo[c + 1])
            r0, r1 = int(goff[g0]), int(goff[g1])
            with StoreBuilder(cr.filters, cr.txp_len) as b:
                b.add_groups(rec[r0:r1], goff[g0:g1 + 1] - goff[g0])
                rp, tid, p, s, e, _ = b.export()
                tables.append(b.discard_table())
            rps.append(rp[1:] + np.uint64(base))
            tids.append(tid)
            ps.append(p)
            ss.append(s)
            es.append(e)
            base += len(tid)
            co[c + 1] = co[c] + np.uint64(len(rp) - 1)
        csr = (co, np.concatenate(rps), np.concatenate(tids), np.concatenate(ps), np.concatenate(ss), np.concatenate(es))
        t_build = time.perf_counter() - t0
        got = em_alone(model, csr)[1]
        return time.perf_counter() - t0, t_build, got, csr

    def em_alone(model, csr):
        co, rp, tid, p, s, e = csr
        t0 = time.perf_counter()
        if model < 0:
            got = oarfish_amd.em_cells_sparse(co, rp, tid, p, None, T)
        else:
            got = oarfish_amd.em_cells_coverage_sparse(co, rp, tid, p, s, e, cr.txp_len, **COV)
        return time.perf_counter() - t0, got

    def differs(got, want):
        """Largest relative difference of a value between two results (same columns asserted)."""
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "columns differ"
        return float(np.max(np.abs(got[2] - want[2]) / np.maximum(np.abs(want[2]), 1e-3))) if len(want[2]) else 0.0

    if args.whitelist_stream:
        whitelist_stream_leg(args, cr, res, save)
        print(json.dumps(res))
        return
    if args.umis_rule_stream:
        umis_rule_stream_leg(args, cr, res, save)
        print(json.dumps(res))
        return
    if args.umis_stream:
        umis_stream_leg(args, cr, res, save)
        print(json.dumps(res))
        return
    if args.barcodes_any_order_stream:
        barcodes_any_order_stream_leg(args, cr, res, save)
        print(json.dumps(res))
        return
    if args.barcodes_stream:
        barcodes_stream_leg(args, cr, res, save)
        print(json.dumps(res))
        return
    if args.whitelist:
        whitelist_leg(args, cr, res, save)
        print(json.dumps(res))
        return
    if args.umis_rule:
        umis_rule_leg(args, cr, res, save)
        print(json.dumps(res))
        return
    if args.umis:
        umis_leg(args, cr, res, save)
        print(json.dumps(res))
        return
    if args.barcodes:
        barcodes_leg(args, cr, res, save)
        print(json.dumps(res))
        return
    if args.names:
        names_leg(args, cr, res, save)
        print(json.dumps(res))
        return
    rate = pinned_rate_gbs()
    res["pinned_h2d_gbs"] = rate
    res["records_pcie_floor_s"] = rec.nbytes / (rate * 1e9)
    save()
    for model in args.models:
        key = "no_coverage" if model < 0 else "binomial_coverage"
        nw = min(args.warm_cells, n)
        one_call(model, nw)
        long_way(model, nw)
        r = res[key] = {}
        runs_a, keep_a = [], None
        for _ in range(args.runs):
            dt, got = one_call(model)
            runs_a.append(dt)
            keep_a = got
        r["one_call_s_runs"], r["one_call_s"] = runs_a, min(runs_a)
        print(f"[bench] {key}: (a) one call {[round(x, 3) for x in runs_a]} s", flush=True)
        save()
        runs_b, builds, csr, keep_b = [], [], None, None
        for _ in range(args.runs):
            dt, tb, got, csr = long_way(model)
            runs_b.append(dt)
            builds.append(tb)
            keep_b = got
        r["long_way_s_runs"], r["long_way_s"] = runs_b, min(runs_b)
        r["long_way_host_builders_s"] = min(builds)
        print(f"[bench] {key}: (b) long way {[round(x, 3) for x in runs_b]} s (builders + export {min(builds):.3f} s)", flush=True)
        r["max_rel_diff_one_call_to_long_way"] = differs(keep_a, keep_b)
        r["alignments_kept"] = int(len(csr[2]))
        save()
        runs_c = [em_alone(model, csr)[0] for _ in range(args.runs)]
        r["em_alone_s_runs"], r["em_alone_s"] = runs_c, min(runs_c)
        print(f"[bench] {key}: (c) EM alone {[round(x, 3) for x in runs_c]} s", flush=True)
        r["speedup_over_long_way"] = r["long_way_s"] / r["one_call_s"]
        r["excess_over_em_alone_s"] = r["one_call_s"] - r["em_alone_s"]
        r["excess_over_pcie_floor"] = r["excess_over_em_alone_s"] / res["records_pcie_floor_s"]
        save()
        del csr, keep_a, keep_b
    # the filter stages of the last group, from HIP events (test-only library, one worker)
    os.environ["OEM_FILTER_TIMING"] = "1"
    os.environ["OEM_CELLS_WORKERS"] = "1"
    with _lib.testing() as L:
        dt, _ = one_call(args.models[0])
        ms = (C.c_float * 6)()
        _lib.check(L.oem_debug_filter_last_timing(ms))
    res["filter_stages_last_group"] = dict(call_s_one_worker=dt, upload_ms=ms[0], k_filter_measure_ms=ms[1], scans_ms=ms[2],
                                           k_filter_emit_ms=ms[3], measure_under_copy_fraction=ms[4], staging_copy_host_ms_all_groups=ms[5])
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
