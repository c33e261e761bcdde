"""The projected session against the one call, at the bench shape ("The projected session").

The input is ``make_projected_records(make_config("c3"))``, similarity source, no coverage model.  In one process and
in alternation, ``--runs`` times each: ``DeviceStore.from_projected_records`` on the whole run, and
``RecordsStream(projected=True)`` fed batches of ``--batch-groups`` groups by ``--threads`` pushing threads (thread t
pushes batches t, t + T, ...).  A session's seconds run from its first push to ``finish`` returning; the share of
``finish`` in them, ``host_finished / nnz`` and the peak of the device memory above the level at entry (first run of
each kind) are recorded beside them.  The result goes to profiles/projected_stream_bench.json.

The per-batch finish of the one call is not timed as a session variant here, so the numbers say nothing about deferred
against per-batch finishing."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oarfish_amd  # noqa: E402,F401
from oarfish_amd import synth  # noqa: E402
from oarfish_amd.builder import RecordsStream  # noqa: E402
from oarfish_amd.types import DeviceStore  # noqa: E402
from cells_records_bench import PeakDeviceMemory, spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-groups", type=int, nargs="+", default=[1 << 18, 1 << 20])
    ap.add_argument("--threads", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reads", type=int, default=0, help="0: the bench shape (c3)")
    ap.add_argument("--txps", type=int, default=200_000)
    ap.add_argument("--warm-groups", type=int, default=200_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "projected_stream_bench.json"))
    args = ap.parse_args()

    t0 = time.perf_counter()
    st = synth.make_store(args.reads, args.txps, threads=16) if args.reads else synth.make_config("c3")
    print(f"[bench] store of {st.n_reads} reads made in {time.perf_counter() - t0:.1f} s", flush=True)
    spr = synth.make_projected_records(st)
    print(f"[bench] {len(spr.records)} projected records made after {time.perf_counter() - t0:.1f} s", flush=True)
    F, tl, kw = spr.filters, spr.txp_len, dict(beta=spr.beta, prob_source="similarity")
    G = len(spr.group_off) - 1
    res = dict(n_reads=int(st.n_reads), n_txps=int(st.n_txps), n_groups=G, n_records=int(len(spr.records)),
               record_bytes=int(spr.records.nbytes), beta=spr.beta, prob_source="similarity", runs=args.runs)

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)

    def one_call(g=G):
        t0 = time.perf_counter()
        store, kept, dt = DeviceStore.from_projected_records(F, tl, spr.records[:int(spr.group_off[g])], spr.group_off[:g + 1],
                                                             spr.read_len[:g], **kw)
        t = time.perf_counter() - t0
        nnz = store.nnz
        store.close()
        return t, kept, dt, nnz

    def session(batches, n_threads):
        errors = []
        with RecordsStream(F, tl, projected=True, **kw) as s:
            def pusher(t):
                try:
                    for r, o, l in batches[t::n_threads]:
                        s.push(r, o, read_len=l)
                except Exception as e:                                  # noqa: BLE001
                    errors.append(e)
            threads = [threading.Thread(target=pusher, args=(t,)) for t in range(n_threads)]
            t0 = time.perf_counter()
            for th in threads:
                th.start()
            for th in threads:
                th.join()
            if errors:
                raise errors[0]
            t1 = time.perf_counter()
            store, kept, dt = s.finish()
            t2 = time.perf_counter()
            info = s.info()
        store.close()
        return t2 - t0, (t2 - t1) / (t2 - t0), kept, dt, info

    one_call(min(args.warm_groups, G))                                  # warm-up on a slice
    legs = [(g, n) for g in args.batch_groups for n in args.threads]
    cut = {g: synth.cut_projected_records(spr, [g] * (G // g)) for g in args.batch_groups}
    a_runs, s_runs = [], {leg: [] for leg in legs}
    for k in range(args.runs):
        if k == 0:
            with PeakDeviceMemory() as pk:
                t_a, want_kept, want_dt, nnz = one_call()
            res["peak_device_bytes_one_call"] = int(pk.peak)
        else:
            t_a, want_kept, want_dt, nnz = one_call()
        a_runs.append(t_a)
        res.update(nnz=int(nnz), one_call=spread(a_runs))
        for g, n in legs:
            q = res.setdefault(f"batch_groups_{g}_threads_{n}", dict(batches=len(cut[g])))
            if k == 0:
                with PeakDeviceMemory() as pk:
                    t_s, share, kept, dt, info = session(cut[g], n)
                q["peak_device_bytes_session"] = int(pk.peak)
                q["peak_session_over_one_call"] = round(q["peak_device_bytes_session"] / max(res["peak_device_bytes_one_call"], 1), 4)
            else:
                t_s, share, kept, dt, info = session(cut[g], n)
            assert dt == want_dt and int(kept.sum()) == int(want_kept.sum())   # (the order of the groups is the tickets')
            if n == 1:
                assert np.array_equal(kept, want_kept)
            s_runs[(g, n)].append(t_s)
            q.update(session=spread(s_runs[(g, n)]), session_over_one_call=round(min(s_runs[(g, n)]) / min(a_runs), 4),
                     finish_share=round(share, 4), host_finished=info["host_finished"],
                     host_finished_over_nnz=round(info["host_finished"] / max(nnz, 1), 6),
                     batches_before_finish=info["batches_before_finish"], blocked_us=info["blocked_us"], host_batches=info["host_batches"])
            save()
            print(f"[bench] run {k}: {g} groups a batch, {n} thread(s): one call {t_a:.3f} s, session {t_s:.3f} s "
                  f"(finish {share:.2f}, host finished {info['host_finished']})", flush=True)
    print(json.dumps({k: v for k, v in res.items() if not isinstance(v, dict) or k == "one_call"}))


if __name__ == "__main__":
    main()
