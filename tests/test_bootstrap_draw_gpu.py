"""GPU tests of WHAT a device-drawn bootstrap replicate is: k_bootstrap_weights (oem_kernels.hip) and the places
that choose which replica a result row draws (oem_bootstrap.hip), against oracle/resample_np.py -- the plain
restatement of the Philox4x32-10 stream of include/oarfish_em.h that tests/test_resample_reference.py pins to the
published known answers.  Weights are compared with np.array_equal on uint32: there is no tolerance.  Replicates are
compared with the oracle's EM over the REFERENCE weights (never over weights fetched from the device) under the rule
of test_batched_bootstrap_matches_oracle_per_replicate: iteration counts at most one apart, counts within 1e-8 where
they agree and within the 1e-4 north star otherwise.

That the tests bite was checked with wrong-number builds of the library (MI355X; "moments" is the earlier, purely
distributional test_device_multinomial_weights):
  nine Philox rounds                     every draw / layout / shard test here fails (n = 1 aside); moments passed
  k1 taken from the seed's low half      the same tests fail; moments passed
  draw 2q+1 built from words (0, 1)      the same tests fail; moments failed too (every multiplicity becomes even)
  `c > 256` in k_pack_row_w_b            the three byte-edge tests fail; moments and the multiplicity-300 test passed
  first_replica + rep + 1, batched site  the batched row tests, the replica-parallel, 2^32 - 1 and tile-variant tests
                                         fail; moments failed too (it compares rows with fetched draws of 0 and 1)
  first_replica + b + 1, one-per-pass    the one-per-pass row tests, the replica-parallel and 2^32 - 1 tests fail;
                                         moments passed
Wall time on an MI355X: 11 s for this file, next to 385 s for tests/test_gpu_parity.py in the same run."""
import functools

import numpy as np
import pytest

from oarfish_amd import _lib, dist as odist, synth
from oarfish_amd.types import DeviceStore
from oracle import c_oracle, resample_np
from tests.common import assert_counts_close, byte_edge_weights

pytestmark = pytest.mark.gpu

RTOL = 1e-4  # north_star tolerance

SEEDS = [0, 11, 0xffffffff, 0x1_0000_0000, 0x123456789abcdef0, 2**64 - 1]
REPLICAS = [0, 1, 4, 2**32 - 1]
# (a, b): the same low half, another high half -- and the reverse
SAME_LOW = [(0, 0x1_0000_0000), (0xffffffff, 2**64 - 1)]
SAME_HIGH = [(0, 11), (11, 0xffffffff), (0x1_0000_0000 + 7, 0x1_0000_0000)]


def _plain_store(n_reads, n_txps):
    """One alignment per read: the draw depends on the read count alone."""
    row_ptr = np.arange(n_reads + 1, dtype=np.uint64)
    tid = (np.arange(n_reads, dtype=np.uint64) % n_txps).astype(np.uint32)
    return row_ptr, tid, np.full(n_reads, 0.5, dtype=np.float32)


def _check_draws(d, n, pairs):
    got = {}
    for seed, replica in pairs:
        w = d.bootstrap_weights(seed, replica)
        want = resample_np.bootstrap_weights(n, seed, replica)
        assert w.dtype == np.uint32 and w.shape == want.shape
        bad = np.nonzero(w != want)[0]
        assert np.array_equal(w, want), (f"n={n} seed={seed:#x} replica={replica}: {len(bad)} reads differ, first "
                                         f"{bad[:5].tolist()}: device {w[bad[:5]].tolist()} reference {want[bad[:5]].tolist()}")
        got[(seed, replica)] = w
    return got


@pytest.mark.parametrize("n_reads", [1, 2, 3, 255, 256, 257, 4_097, 200_001, 1_000_000])
def test_draw_equals_the_reference_stream_bit_for_bit(n_reads):
    """Odd and even stores (the cut last pair), fewer draws than one workgroup, and 1 000 000 reads = 500 000 counter
    blocks, which is less than the grid cap (the 10 M store below is above it).  Every seed x replica: both key halves, the
    replica word at its extremes."""
    row_ptr, tid, p = _plain_store(n_reads, 1000)
    pairs = [(s, r) for s in SEEDS for r in REPLICAS]
    with DeviceStore(row_ptr, tid, p, None, 1000) as d:
        got = _check_draws(d, n_reads, pairs + [(0x1_0000_0000 + 7, 0)])
    if n_reads >= 255:   # (a store of 1-3 reads has a handful of possible draws)
        for a, b in SAME_LOW + SAME_HIGH:
            assert not np.array_equal(got[(a, 0)], got[(b, 0)]), f"seeds {a:#x} and {b:#x} draw the same resample"
        for s in SEEDS:
            for i, r in enumerate(REPLICAS):
                for r2 in REPLICAS[:i]:
                    assert not np.array_equal(got[(s, r)], got[(s, r2)]), (hex(s), r, r2)


def test_draw_of_ten_million_reads_runs_the_grid_stride_loop():
    """5 000 000 counter blocks against a grid capped at 4096 x 256 threads: every thread draws several blocks, and
    the block index is far past 2^20.  One store, three streams."""
    n = 10_000_000
    row_ptr, tid, p = _plain_store(n, 200_000)
    with DeviceStore(row_ptr, tid, p, None, 200_000) as d:
        _check_draws(d, n, [(11, 0), (0x123456789abcdef0, 4), (2**64 - 1, 2**32 - 1)])


@pytest.mark.parametrize("layout_build", [0, 1])
@pytest.mark.parametrize("reorder_rows", [0, 1, 2])
def test_draw_is_in_caller_order_whatever_the_layout(reorder_rows, layout_build):
    st = synth.make_store(20_007, 900, seed=23)
    with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, st.n_txps, reorder_rows=reorder_rows,
                     layout_build=layout_build) as d:
        _check_draws(d, st.n_reads, [(0x123456789abcdef0, 1), (11, 2**32 - 1)])


def _slice_rows(st, b, e):
    a0, a1 = int(st.row_ptr[b]), int(st.row_ptr[e])
    return (st.row_ptr[b:e + 1] - st.row_ptr[b]).astype(np.uint64), st.tid[a0:a1], st.as_prob[a0:a1]


@pytest.mark.parametrize("split", ["nnz2", "nnz3", "nnz7", "odd_cuts"])
def test_row_shard_draws_its_window_of_the_reference_stream(split):
    """A shard [row_begin, row_begin + n_local) of n_global reads (1-rank communicator, as in
    test_row_shard_semantics_single_rank): n_global != n_local, local_off != 0.  The hand-made split has odd
    boundaries and two shards of a single read."""
    st = synth.make_store(80_001, 5_000, seed=300)
    n = st.n_reads
    if split == "odd_cuts":
        cuts = [0, 1, 33_333, 33_334, 80_001]
        bounds = list(zip(cuts[:-1], cuts[1:]))
    else:
        bounds = odist.shard_bounds_by_nnz(st.row_ptr, int(split[3:]))
    assert bounds[0][0] == 0 and bounds[-1][1] == n and all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))
    comm = odist.create_comm(0, 1, 0)
    try:
        for seed, replica in [(0xfeedface_00000011, 1), (42, 2**32 - 1)]:
            parts = []
            for b, e in bounds:
                row_ptr, tid, p = _slice_rows(st, b, e)
                with DeviceStore(row_ptr, tid, p, None, st.n_txps) as d:
                    d.attach_comm(comm.handle, n, b)
                    w = d.bootstrap_weights(seed, replica)
                want = resample_np.bootstrap_weights(n, seed, replica, b, e - b)
                assert np.array_equal(w, want), (split, hex(seed), replica, b, e)
                parts.append(w)
            assert int(np.concatenate(parts).sum()) == n
    finally:
        comm.close()


# ---------------------------------------------------------------------------
# which replica each output row is
# ---------------------------------------------------------------------------
BOOT_SEED = 0x9e3779b9_0000002a   # both key halves in use
BOOT_ITERS = 300


@functools.lru_cache(maxsize=None)
def _boot_store():
    st = synth.make_store(40_000, 2_500, seed=81)
    return st, c_oracle.Store(st.row_ptr, st.tid, st.as_prob, None, st.n_txps)


@functools.lru_cache(maxsize=None)
def _oracle_replica(replica):
    st, o = _boot_store()
    return c_oracle.do_em(o, row_w=resample_np.bootstrap_weights(st.n_reads, BOOT_SEED, replica), max_iter=BOOT_ITERS,
                          conv_thresh=1e-3)


def _assert_replicate(got, info, want_info, n_reads, n_txps, what):
    want, wi = want_info
    assert abs(info.niter - wi.niter) <= 1, (what, info, wi)
    same = info.niter == wi.niter
    if same:
        assert info.n_passes == wi.n_passes and info.converged == wi.converged, (what, info, wi)
    assert_counts_close(got, want, n_reads, n_txps, 1e-8 if same else RTOL, what)


def _differ(a, b, n_reads, n_txps):
    try:
        assert_counts_close(a, b, n_reads, n_txps, RTOL)
    except AssertionError:
        return True
    return False


def test_neighbouring_replicas_are_distinguishable_by_the_acceptance_rule():
    """The guard of the tests below, on the oracle side alone: a row that held the replicate of replica b - 1 or
    b + 1 would not pass for replica b.  Measured on the CPU for this store and seed, replicas 0..25: between any
    two neighbouring replicas at least 49.6 % of the 2500 transcripts differ by more than RTOL (in the most alike
    pair), and the worst transcript of that pair differs by 1.2e5 relative to the floored count -- nine orders above
    RTOL.  No two of the 26 replicas, neighbours or not, pass for each other."""
    st, _ = _boot_store()
    res = [_oracle_replica(b)[0] for b in range(26)]
    for a in range(26):
        for b in range(26):
            if a != b:
                assert _differ(res[a], res[b], st.n_reads, st.n_txps), (a, b)
    for b in range(25):
        far = np.abs(res[b] - res[b + 1]) > RTOL * np.maximum(np.abs(res[b + 1]), 1e-5 * st.n_reads / st.n_txps)
        assert far.mean() > 0.25, (b, far.mean())


@pytest.mark.parametrize("batch", [1, 0])
@pytest.mark.parametrize("b0", [0, 5])
def test_each_bootstrap_row_is_the_replicate_of_its_own_replica(b0, batch):
    """oem_bootstrap, weights drawn on the device: row b is the EM over the resample of global replica b0 + b --
    with 21 replicates handed out from one counter to two chains of four slots (slots refilled, an idle tail), and
    one per pass."""
    st, _ = _boot_store()
    n_boot = 21
    with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, st.n_txps) as d:
        d.set_option(_lib.OEM_OPT_BATCH_BOOTSTRAP, batch)
        out, infos = d.bootstrap(n_boot, seed=BOOT_SEED, max_iter=BOOT_ITERS, conv_thresh=1e-3, first_replica=b0)
    for b in range(n_boot):
        _assert_replicate(out[b], infos[b], _oracle_replica(b0 + b), st.n_reads, st.n_txps,
                          f"b0={b0} batch={batch} row {b} (replica {b0 + b})")


def test_replica_parallel_rank_draws_its_own_replica():
    """odist.bootstrap_replica_parallel: rank 2 of 5 over 5 replicates runs the one replicate of replica 2;
    rank 1 of 2 runs replicas 2..4."""
    st, _ = _boot_store()
    with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, st.n_txps) as d:
        b0, out, infos = odist.bootstrap_replica_parallel(d, 5, BOOT_SEED, 2, 5, max_iter=BOOT_ITERS)
        assert (b0, len(out)) == (2, 1)
        _assert_replicate(out[0], infos[0], _oracle_replica(2), st.n_reads, st.n_txps, "rank 2 of 5")
        b0, out, infos = odist.bootstrap_replica_parallel(d, 5, BOOT_SEED, 1, 2, max_iter=BOOT_ITERS)
        assert (b0, len(out)) == (2, 3)
        for k in range(3):
            _assert_replicate(out[k], infos[k], _oracle_replica(2 + k), st.n_reads, st.n_txps, f"rank 1 of 2, row {k}")


def test_replica_index_past_32_bits_is_an_argument_error():
    """include/oarfish_em.h: the replica word of the stream is 32 bits; a call whose last replicate would draw a
    replica past 2^32 - 1 is refused (OEM_ERR_ARG) instead of wrapping onto replica 0.  The last representable
    replicas still run, batched and alone, and are the replicates of those replicas."""
    st, o = _boot_store()
    top = 2**32 - 1
    with DeviceStore(st.row_ptr, st.tid, st.as_prob, None, st.n_txps) as d:
        for n_boot, first in [(2, top), (3, top - 1), (21, top - 19)]:
            with pytest.raises(_lib.OemError) as ei:
                d.bootstrap(n_boot, seed=BOOT_SEED, max_iter=BOOT_ITERS, first_replica=first)
            assert ei.value.code == _lib.OEM_ERR_ARG, ei.value
        with pytest.raises(_lib.OemError):
            d.bootstrap(1, seed=BOOT_SEED, max_iter=BOOT_ITERS, first_replica=top + 1)
        one, i1 = d.bootstrap(1, seed=BOOT_SEED, max_iter=BOOT_ITERS, first_replica=top)
        two, i2 = d.bootstrap(2, seed=BOOT_SEED, max_iter=BOOT_ITERS, first_replica=top - 1)
        # injected weights draw nothing: the option does not bear on them
        w = resample_np.bootstrap_weights(st.n_reads, BOOT_SEED, 0)
        inj, i3 = d.bootstrap(2, row_w_all=np.stack([w, w]), max_iter=BOOT_ITERS, first_replica=top)
    want = {r: c_oracle.do_em(o, row_w=resample_np.bootstrap_weights(st.n_reads, BOOT_SEED, r), max_iter=BOOT_ITERS,
                              conv_thresh=1e-3) for r in (top - 1, top)}
    assert _differ(want[top][0], want[top - 1][0], st.n_reads, st.n_txps)
    assert _differ(want[top][0], _oracle_replica(0)[0], st.n_reads, st.n_txps)
    _assert_replicate(one[0], i1[0], want[top], st.n_reads, st.n_txps, "replica 2^32-1 alone")
    _assert_replicate(two[0], i2[0], want[top - 1], st.n_reads, st.n_txps, "replica 2^32-2")
    _assert_replicate(two[1], i2[1], want[top], st.n_reads, st.n_txps, "replica 2^32-1")
    for k in range(2):
        _assert_replicate(inj[k], i3[k], _oracle_replica(0), st.n_reads, st.n_txps, f"injected row {k}")


# ---------------------------------------------------------------------------
# the byte edge of the batched replicates' multiplicities
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["coverage_f64", "f32_stream", "fused"])
def test_multiplicities_at_the_byte_edge_match_the_oracle(kind):
    """k_pack_row_w_b carries a batched replicate's multiplicities as bytes and hands a replicate with one >= 256
    to the one-per-pass path: 255 must stay exact, 256 must not wrap to 0 -- alone, next to a 255, and with
    ordinary replicates around them in the two chains.  Every row against the oracle on the same weights; with
    max_iter = 1 every row leaves through max_iter after two passes.  The batch kernel is instantiated for f64
    (coverage) and f32 weights, streamed or dictionary-coded."""
    st = synth.make_store(40_000, 2_500, seed=81, coverage=kind == "coverage_f64")
    o = c_oracle.Store(st.row_ptr, st.tid, st.as_prob, st.cov_prob, st.n_txps)
    W, names = byte_edge_weights(st.n_reads, seed=0x5eed_0000_0001)
    assert int(W[1].max()) == 255 and int(W[3].max()) == 256 and int(W[5].max()) == 255
    assert int(W[[0, 2, 6]].max()) < 64 and {255, 256} <= set(np.unique(W[4]).tolist())
    with DeviceStore(st.row_ptr, st.tid, st.as_prob, st.cov_prob, st.n_txps,
                     weight_coding=1 if kind == "f32_stream" else 0) as d:
        if kind != "coverage_f64":
            assert (d.info(_lib.OEM_INFO_WEIGHT_DICT_ENTRIES) > 0) == (kind == "fused")
        d.set_option(_lib.OEM_OPT_BATCH_BOOTSTRAP, 1)
        out, infos = d.bootstrap(len(W), row_w_all=W, max_iter=200, conv_thresh=1e-3)
        out1, infos1 = d.bootstrap(len(W), row_w_all=W, max_iter=1, conv_thresh=1e-3)
        # the 255 replicates without a fallback replicate in the call
        keep = [0, 1, 5, 2, 6]
        out2, infos2 = d.bootstrap(len(keep), row_w_all=W[keep], max_iter=200, conv_thresh=1e-3)
    for b in range(len(W)):
        want = c_oracle.do_em(o, row_w=W[b], max_iter=200, conv_thresh=1e-3)
        _assert_replicate(out[b], infos[b], want, st.n_reads, st.n_txps, f"{kind} replicate {b} ({names[b]})")
        if b in keep:
            k = keep.index(b)
            _assert_replicate(out2[k], infos2[k], want, st.n_reads, st.n_txps, f"{kind} no-fallback call, {names[b]}")
        want1 = c_oracle.do_em(o, row_w=W[b], max_iter=1, conv_thresh=1e-3)
        assert infos1[b].niter == 1 and infos1[b].n_passes == 2, (kind, b, infos1[b])
        _assert_replicate(out1[b], infos1[b], want1, st.n_reads, st.n_txps, f"{kind} max_iter=1 replicate {b} ({names[b]})")
