#!/usr/bin/env python
"""The bulk parser on the device (oem_store_create_records_names, DeviceStore.from_named_records) against the hand join
it replaces, at the bench shape: synth.make_config("c3") (10 M reads, 200 k transcripts) through synth.make_records and
synth.make_named_records, 83.7 M records, per name style (UUID, Illumina-style):

  (a) the one call: ADJACENT on the collated input, and SORT on the same input permuted;
  (b) the hand join, by stage: collate_names on the names as one cell, the NumPy gather records[order], from_records;
  (c) from_records on input that has its group_off already: the floor of the upload and filter part;
  the PCIe floor of records plus names at the pinned host-to-device rate measured here, and the peak of the device
  memory in use during (a), sampled from another thread.

A warm-up on a slice, then --runs repeats (default five) of (a), (b), (c) in alternation; best and worst of each,
(a) - (c) -- what the names cost on the device -- and (a) / (b).  The result goes to --out as JSON, rewritten after every
measurement.  --reads / --txps shrink the shape for a trial run.

--stream is the names session's leg instead (RecordsStream(names=True), oem_records_stream_push_names): the same input
cut at record positions into batches of 2^18 and of 2^20 groups' worth of records (--batch-groups), pushed from one
thread; seconds from the first push to the end of finish, beside the one call (ADJACENT) timed in the same run, --runs
repeats in alternation, and for both the peak of the device memory above the level at entry.  The result goes to
profiles/records_names_stream_bench.json.

--stream --sort is the sorting names session's leg (RecordsStream(names=True, mode="sort"),
oem_records_stream_push_sort): the same input PERMUTED, with its secondary flags, in the same batches, beside the one
call with mode="sort" on the permuted input; order, kept and the discard table are compared in every run, and the
arena's peak (info()["arena_bytes"]) is recorded.  The result goes to profiles/records_names_sort_stream_bench.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oarfish_amd  # noqa: E402
from oarfish_amd import synth  # noqa: E402
from oarfish_amd.builder import RecordsStream  # noqa: E402
from oarfish_amd.types import DeviceStore  # noqa: E402
from cells_records_bench import PeakDeviceMemory, pinned_rate_gbs, spread  # noqa: E402


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def drop_unmapped(R, B, O, S):
    """Step 1 of the hand join: the unmapped records, their names and flags dropped on the host (boolean masks)."""
    keep = (R["flags"] & 1) == 0
    if keep.all():
        return (B, O), S, R
    lens = np.diff(O).astype(np.int64)
    off = np.zeros(int(keep.sum()) + 1, dtype=np.uint64)
    np.cumsum(lens[keep], out=off[1:])
    return (B[np.repeat(keep, lens)], off), S[keep], R[keep]


def close(result):
    result[0].close()
    return result[1:]


def stream_leg(args, sr, res, save):
    """The --stream leg (see the module docstring); fills res[style]["batch_groups_<g>"]."""
    F, tl = sr.filters, sr.txp_len
    n_groups = len(sr.group_off) - 1
    for style in args.styles:
        rec, (blob, off), sec = synth.make_named_records(sr, style=style, unmapped_rate=args.unmapped_rate, shuffle=args.sort)
        n = len(rec)
        r = res[style] = dict(record_bytes=int(rec.nbytes), name_bytes=int(blob.nbytes))

        def one_call(m=n):
            if args.sort:   # (the parse comes back too: its order is compared with the session's)
                out = DeviceStore.from_named_records(F, tl, rec[:m], (blob[:int(off[m])], off[:m + 1]), secondary=sec[:m], mode="sort")
                return close(out[:3]) + (out[3].order,)
            return close(DeviceStore.from_named_records(F, tl, rec[:m], (blob[:int(off[m])], off[:m + 1]),
                                                        sort_check_num=0 if m < n else 100_000))

        one_call(min(args.warm_records, n))                      # warm-up on a slice
        for g in args.batch_groups:
            per = max(1, int(round(g * n / max(n_groups, 1))))   # records per batch: g groups' worth, cut at record positions
            edges = list(range(0, n, per)) + [n]
            batches = [(rec[a:b], (blob[int(off[a]):int(off[b])], off[a:b + 1] - off[a]), sec[a:b] if args.sort else None)
                       for a, b in zip(edges[:-1], edges[1:])]
            q = r[f"batch_groups_{g}"] = dict(records_per_batch=per, batches=len(batches))

            def session():
                with RecordsStream(F, tl, names=True, mode="sort" if args.sort else "adjacent") as s:
                    t0 = time.perf_counter()
                    for b_rec, b_names, b_sec in batches:
                        s.push(b_rec, names=b_names, secondary=b_sec)
                    store, kept, dt, parse = s.finish()
                    t = time.perf_counter() - t0
                    info = s.info()
                store.close()
                if args.sort:
                    info["order"] = parse.order
                return t, kept, dt, info

            a_runs, s_runs = [], []
            for k in range(args.runs):
                if k == 0:
                    with PeakDeviceMemory() as pk:
                        t_a, got = clock(one_call)
                    q["peak_device_bytes_one_call"] = int(pk.peak)
                    with PeakDeviceMemory() as pk:
                        t_s, kept, dt, info = session()
                    q["peak_device_bytes_session"] = int(pk.peak)
                else:
                    t_a, got = clock(one_call)
                    t_s, kept, dt, info = session()
                assert np.array_equal(kept, got[0]) and dt == got[1]              # kept and the discard table agree
                if args.sort:                                                     # ... and so does the collated order
                    assert np.array_equal(info.pop("order"), got[2].astype(np.int64))
                    q["arena_bytes"] = info["arena_bytes"]
                a_runs.append(t_a)
                s_runs.append(t_s)
                q.update(one_call=spread(a_runs), session=spread(s_runs), session_over_one_call=round(min(s_runs) / min(a_runs), 4),
                         batches_before_finish=info["batches_before_finish"], blocked_us=info["blocked_us"], host_batches=info["host_batches"])
                q["peak_session_over_one_call"] = round(q["peak_device_bytes_session"] / max(q["peak_device_bytes_one_call"], 1), 4)
                save()
                print(f"[bench] {style} {g} groups a batch, run {k}: one call {t_a:.3f} s, session {t_s:.3f} s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stream", action="store_true", help="the names session against the one call (see the module docstring)")
    ap.add_argument("--sort", action="store_true", help="with --stream: the sorting names session on permuted input against the one call's mode=\"sort\"")
    ap.add_argument("--batch-groups", type=int, nargs="+", default=[1 << 18, 1 << 20])
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--styles", nargs="+", default=["uuid", "illumina"])
    ap.add_argument("--reads", type=int, default=0, help="0: the bench shape (c3)")
    ap.add_argument("--txps", type=int, default=200_000)
    ap.add_argument("--unmapped-rate", type=float, default=0.0)
    ap.add_argument("--warm-records", type=int, default=2_000_000)
    args = ap.parse_args()
    if args.sort and not args.stream:
        ap.error("--sort belongs to --stream")
    if args.out is None:
        name = "records_names_sort_stream_bench.json" if args.sort else "records_names_stream_bench.json" if args.stream else "records_names_bench.json"
        args.out = os.path.join(ROOT, "profiles", name)

    st = synth.make_store(args.reads, args.txps, threads=16) if args.reads else synth.make_config("c3")
    sr = synth.make_records(st)
    F, tl = sr.filters, sr.txp_len
    res = dict(n_reads=int(st.n_reads), n_txps=int(st.n_txps), n_records=int(len(sr.records)), runs=args.runs,
               unmapped_rate=args.unmapped_rate, pinned_h2d_gbs=round(pinned_rate_gbs(), 2))

    if os.path.exists(args.out):      # a run per name style may add to the file of an earlier one at the same shape
        old = json.load(open(args.out))
        if all(old.get(k) == res[k] for k in ("n_reads", "n_txps", "n_records", "unmapped_rate")):
            res.update({k: v for k, v in old.items() if isinstance(v, dict) and k not in args.styles})

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)

    if args.stream:
        stream_leg(args, sr, res, save)
        print(json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}))
        return
    for style in args.styles:
        rec, (blob, off), sec = synth.make_named_records(sr, style=style, unmapped_rate=args.unmapped_rate)
        rec_p, (blob_p, off_p), sec_p = synth.make_named_records(sr, style=style, unmapped_rate=args.unmapped_rate, shuffle=True)
        n = len(rec)
        r = res[style] = dict(record_bytes=int(rec.nbytes), name_bytes=int(blob.nbytes))
        r["pcie_floor_s"] = round((rec.nbytes + blob.nbytes + off.nbytes) / (res["pinned_h2d_gbs"] * 1e9), 4)
        group_off_known = None

        def one_call(m=n, permuted=False):
            if permuted:
                return close(DeviceStore.from_named_records(F, tl, rec_p[:m], (blob_p[:int(off_p[m])], off_p[:m + 1]), secondary=sec_p[:m],
                                                            mode="sort"))
            return close(DeviceStore.from_named_records(F, tl, rec[:m], (blob[:int(off[m])], off[:m + 1]), secondary=sec[:m], sort_check_num=0
                                                        if m < n else 100_000))

        def hand_join(permuted=False):
            R, B, O, S = (rec_p, blob_p, off_p, sec_p) if permuted else (rec, blob, off, sec)
            t_d, (nm, sc, rr) = clock(lambda: drop_unmapped(R, B, O, S))
            t_c, (order, goff, _) = clock(lambda: oarfish_amd.collate_names(nm, [0, len(rr)], secondary=sc, mode="sort" if permuted else "adjacent"))
            t_g, sorted_rec = clock(lambda: rr[order])
            t_f, out = clock(lambda: close(DeviceStore.from_records(F, tl, sorted_rec, goff)))
            return dict(drop_unmapped_s=t_d, collate_names_s=t_c, gather_s=t_g, from_records_s=t_f), out, (sorted_rec, goff)

        one_call(min(args.warm_records, n))                      # warm-up on a slice (a read may be cut at its end: no check)
        a_adj, a_sort, b_adj, b_sort, c_runs, stages = [], [], [], [], [], []
        for k in range(args.runs):
            if k == 0:
                with PeakDeviceMemory() as pk:
                    dt, got = clock(one_call)
                r["peak_device_bytes_adjacent"] = int(pk.peak)
                with PeakDeviceMemory() as pk:
                    dt_s, got_s = clock(lambda: one_call(permuted=True))
                r["peak_device_bytes_sort"] = int(pk.peak)
            else:
                dt, got = clock(one_call)
                dt_s, got_s = clock(lambda: one_call(permuted=True))
            a_adj.append(dt)
            a_sort.append(dt_s)
            st_b, out_b, group_off_known = hand_join()
            b_adj.append(sum(st_b.values()))
            stages.append({k2: round(v, 4) for k2, v in st_b.items()})
            st_p, out_p, _ = hand_join(permuted=True)
            b_sort.append(sum(st_p.values()))
            c_runs.append(clock(lambda: close(DeviceStore.from_records(F, tl, *group_off_known)))[0])
            assert np.array_equal(got[0], out_b[0]) and got[1] == out_b[1]           # kept and the discard table agree
            assert np.array_equal(got_s[0], out_p[0]) and got_s[1] == out_p[1]
            r.update(a_adjacent=spread(a_adj), a_sort=spread(a_sort), b_adjacent=spread(b_adj), b_sort=spread(b_sort),
                     b_adjacent_stages=stages, c_from_records=spread(c_runs))
            r["a_minus_c_s"] = round(min(a_adj) - min(c_runs), 4)
            r["a_over_b_adjacent"] = round(min(a_adj) / min(b_adj), 4)
            r["a_over_b_sort"] = round(min(a_sort) / min(b_sort), 4)
            r["a_is_below_b"] = bool(min(a_adj) < min(b_adj) and min(a_sort) < min(b_sort))
            save()
            print(f"[bench] {style} run {k}: (a) {dt:.3f} s adjacent, {dt_s:.3f} s sort; (b) {b_adj[-1]:.3f} / {b_sort[-1]:.3f} s; (c) {c_runs[-1]:.3f} s",
                  flush=True)
    print(json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}))


if __name__ == "__main__":
    main()
