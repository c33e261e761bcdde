#!/usr/bin/env python3
"""One rank of the multi-PROCESS test of the rel_diff record of a row-sharded run (tests/test_run_history_gpu.py):
launched under torch.distributed.run with `gloo`, every rank on cuda:0, the exchange peer to peer and fused into the
rel-diff kernel (k_p2p_reldiff, oem_p2p.hip).  Every rank records; rank 0 gathers the histories and checks that they
are bitwise identical on every rank, within the tolerance of the oracle loop's, and as long as the un-sharded run's.
usage: run_history_worker.py <out.json>"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch                      # noqa: E402
import torch.distributed as dist  # noqa: E402

from oarfish_amd import _lib, dist as odist, synth  # noqa: E402
from oarfish_amd.types import DeviceStore            # noqa: E402

out_path = sys.argv[1]
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group("gloo")
st = synth.make_store(60_000, 3_000, seed=4711, threads=2)
T = st.n_txps
RUNS = [(400, 1e-3, 50), (400, 1e-3, 1), (60, 0.0, 50)]
sh = odist.shard_rows_by_nnz(st.row_ptr, st.tid, st.as_prob, None, rank, world)
res, err = {}, None
try:
    with DeviceStore(sh.row_ptr, sh.tid, sh.as_prob, None, T, device=0) as d:
        comm = odist.create_comm(rank, world, 0, backend="p2p", p2p_capacity=2 * T * 4)
        try:
            d.attach_comm(comm.handle, st.n_reads, sh.row_begin)
            res["runs"] = []
            for m, th, g in RUNS:
                d.set_option(_lib.OEM_OPT_RUN_HISTORY, m)
                _cnt, info = d.em_run(None, m, th, g)
                res["runs"].append((info, d.run_history(0), d.run_history_len(0)))
        finally:
            comm.close()
except Exception as e:   # every rank must reach the gather
    err = repr(e)
gathered = [None] * world
dist.gather_object((err, res), gathered if rank == 0 else None, dst=0)
ok, report = True, {}
if rank == 0:
    errs = [g[0] for g in gathered if g[0]]
    if errs:
        ok, report = False, {"errors": errs}
    else:
        from oracle import c_oracle
        from tests.run_history_common import check_history, oracle_history
        rs = [g[1]["runs"] for g in gathered]
        try:
            o = c_oracle.Store(st.row_ptr, st.tid, st.as_prob, None, T)
            with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, T) as full:
                for k, (m, th, g) in enumerate(RUNS):
                    want = oracle_history(o, st.n_reads, None, m, th, g)
                    _, wi = c_oracle.do_em(o, max_iter=m, conv_thresh=th, min_iter_gate=g)
                    assert (want[1], want[2]) == (wi.niter, wi.converged), (k, want[1:], wi)
                    full.set_option(_lib.OEM_OPT_RUN_HISTORY, m)
                    full.em_run(None, m, th, g)
                    assert full.run_history_len(0) == rs[0][k][2], (k, full.run_history_len(0), rs[0][k][2])
                    for r in range(world):
                        info, hist, n = rs[r][k]
                        assert hist.tobytes() == rs[0][k][1].tobytes(), f"run {k}: rank {r} differs from rank 0"
                        check_history(hist, n, info, want, f"world {world}, rank {r}, run {k}")
            report = {"world": world, "lengths": [int(x[2]) for x in rs[0]]}
        except AssertionError as e:
            ok, report = False, {"assertion": repr(e)[:2000]}
    json.dump({"ok": ok, **report}, open(out_path, "w"))
    print("run-history worker:", "OK" if ok else "FAIL", report)
dist.barrier()
dist.destroy_process_group()
sys.exit(0 if ok else 1)
