"""GPU tests of the remote folds -- k_remote_fold, k_remote_fold_b, k_multi_fold_reldiff -- and of the lane-level run sums
they share (oarfish_amd/csrc/oem_lane_runs.h) on crafted queues, through the hooks of the test-only library.

A fold is a scatter-add: entry i of bucket b goes into cnt[b * 4096 + q_dst[i]].  With integer-valued doubles every
order of summation gives the same bits, so the reference is numpy's add.at in float64 and the comparison is equality of
bit patterns, touched and untouched elements alike.  A second, small set of lognormal values is held to the worst-case
reordering bound (n - 1) 2^-53 sum|v| per destination."""
import numpy as np
import pytest

from oarfish_amd import _lib

pytestmark = pytest.mark.gpu

K_BUCKET = 4096          # oem_layout.h: transcripts per remote bucket
K_BATCH = 4              # oem_internal.h: slots of one chain of the batched bootstrap
RUNNING, FINAL, FINISHED = 0, 1, 2
MIN_READ_THRESH = 1e-5   # include/oarfish_em.h
U = 2.0 ** -53


def _p(a):
    return a.ctypes.data


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _ok(rc):
    assert rc == 0, _lib.testing_lib().oem_last_error()


# ------------------------------------------------------------------------------------------------------------------
# lane level: keys_repeat<stride> and sum_runs_of_equal_keys<stride, stride>
# ------------------------------------------------------------------------------------------------------------------

def lane_runs(stride, keys, vals, n_active=64):
    """keys [W, 64], vals [W, 64, stride] -> (values after the call [W, 64, stride], keys_repeat per wave [W])"""
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    vals = np.ascontiguousarray(vals, dtype=np.float64)
    W = keys.shape[0]
    assert keys.shape == (W, 64) and vals.shape == (W, 64, stride)
    out = np.full(vals.shape, np.nan)
    rep = np.full(W, 99, dtype=np.uint32)
    _ok(_lib.testing_lib().oem_test_lane_runs(stride, _p(keys), _p(vals), W, n_active, _p(out), _p(rep), 0))
    return out, rep


def lane_reference(stride, keys, vals, n_active=64):
    """The contract.  A run = a maximal stretch of active lanes `stride` apart, inside one row of 16, with equal keys; its
    last lane holds the sum of the run's inputs, its other lanes 0.0; lanes >= n_active keep their input.  Returns the
    values, the number of active lanes that equal their neighbour `stride` down the row, and the number of runs."""
    W, E = keys.shape[0], 16 // stride
    k = np.asarray(keys, dtype=np.uint32).reshape(W, 4, E, stride)          # [wave, row, entry, lane of the entry]
    v = np.asarray(vals, dtype=np.float64).reshape(W, 4, E, stride, stride)
    act = np.broadcast_to(np.arange(64).reshape(4, E, stride) < n_active, k.shape)
    head = np.ones(k.shape, dtype=bool)
    head[:, :, 1:, :] = k[:, :, 1:, :] != k[:, :, :-1, :]
    run = np.cumsum(head, axis=2) - 1
    chain = (np.arange(W)[:, None, None, None] * 4 + np.arange(4)[None, :, None, None]) * stride + np.arange(stride)[None, None, None, :]
    gid = chain * E + run
    sums = np.stack([np.bincount(gid[act], weights=v[act][:, j], minlength=W * 4 * stride * E) for j in range(stride)], axis=1)
    last = np.ones(k.shape, dtype=bool)
    last[:, :, :-1, :] = head[:, :, 1:, :] | ~act[:, :, 1:, :]
    want = np.where(last[..., None], sums[gid], 0.0)
    want = np.where(act[..., None], want, v)
    n_equal = (~head & act).reshape(W, -1).sum(axis=1)
    return want.reshape(W, 64, stride), n_equal, int((head & act).sum())


def lane_values(W, stride):
    """Distinct integer-valued doubles: the lane's bit of its row plus a multiple of 2^16 that names the row, so a sum
    says which lanes went into it, how many, and from which row.  The second value of a stride-2 lane is another number."""
    lane = np.arange(64)
    v0 = (1 << (lane % 16)).astype(np.float64) + 65536.0 * (lane // 16 + 1)
    vals = np.empty((W, 64, stride))
    vals[:, :, 0] = v0[None, :] + 2.0 ** 20 * (np.arange(W) % 8)[:, None]
    if stride == 2:
        vals[:, :, 1] = 3.0 * v0[None, :] + 2.0 ** 24 + 7.0 * (lane + 1)[None, :]
    return vals


def keys_of_heads(heads):
    """heads [..., E] booleans (entry 0 is a head whatever it says) -> key = run index mod 2: equal keys recur two runs apart"""
    h = np.array(heads, dtype=np.int64)
    h[..., 0] = 1
    return ((np.cumsum(h, axis=-1) - 1) % 2).astype(np.uint32)


def assert_lanes(stride, keys, vals, n_active=64, check_repeat=True):
    got, rep = lane_runs(stride, keys, vals, n_active)
    want, n_equal, n_runs = lane_reference(stride, keys, vals, n_active)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, (f"stride {stride}, n_active {n_active}: {len(bad)} values differ, first (wave, lane, value) {bad[0]}: "
                           f"keys {keys[bad[0][0]].tolist()} got {got[bad[0][0], :, bad[0][2]].tolist()} "
                           f"want {want[bad[0][0], :, bad[0][2]].tolist()}")
    if check_repeat:
        assert rep.tolist() == (n_equal >= 16).astype(np.uint32).tolist(), (stride, n_active, n_equal.tolist(), rep.tolist())
    return n_runs, n_equal


def test_lane_runs_every_head_pattern_of_a_row_stride_1():
    """All 2^15 ways to cut a row of 16 lanes into runs (lane 0 always starts one), four rows to a wave; the keys alternate
    0 1 0 1 from run to run, so keys two runs apart are equal and only the head flags keep them apart."""
    n_pat = 1 << 15
    W = n_pat // 4
    pat = (np.arange(W)[:, None] + W * np.arange(4)[None, :])                 # the four rows of a wave differ in the high bits
    heads = np.concatenate([np.ones((W, 4, 1), dtype=np.int64), (pat[:, :, None] >> np.arange(15)) & 1], axis=2)
    keys = keys_of_heads(heads).reshape(W, 64)
    n_runs, _ = assert_lanes(1, keys, lane_values(W, 1))
    n_cases = len(np.unique(pat))
    assert n_cases == n_pat                                                   # (the grid did not collapse: every pattern once)
    assert n_runs == n_pat + 15 * n_pat // 2                                  # 1 + (15 free heads, half of them set) per row


def test_lane_runs_every_entry_pattern_of_a_row_stride_2():
    """All 2^7 ways to cut the 8 entries of a row into runs, for the even lanes and -- in another order -- for the odd
    lanes: the two lanes of an entry carry different keys and different values, two values each."""
    n_pat = 1 << 7
    W = n_pat // 4
    pat_even = (np.arange(W)[:, None] + W * np.arange(4)[None, :])
    pat_odd = (pat_even * 37 + 11) % n_pat
    keys = np.empty((W, 4, 8, 2), dtype=np.uint32)
    for par, pat in ((0, pat_even), (1, pat_odd)):
        heads = np.concatenate([np.ones((W, 4, 1), dtype=np.int64), (pat[:, :, None] >> np.arange(7)) & 1], axis=2)
        keys[:, :, :, par] = keys_of_heads(heads) + 2 * par                   # (odd lanes: keys 2 and 3)
    n_runs, _ = assert_lanes(2, keys.reshape(W, 64), lane_values(W, 2))
    n_cases = len(np.unique(pat_even)) + len(np.unique(pat_odd))
    assert n_cases == 2 * n_pat                                               # (the grid did not collapse)
    assert n_runs == 2 * (n_pat + 7 * n_pat // 2)


def partial_wave_keys(stride, n_active, rng):
    """One run per row; all singletons; a run that ends exactly at n_active (the lanes behind it carry the same key: only
    the exec mask ends the run); the same with a singleton in front; random cuts."""
    lane = np.arange(64)
    one_run = np.full(64, 7, dtype=np.uint32)
    singles = (lane + 100).astype(np.uint32)
    ends = singles.copy()
    ends[max(0, n_active - 5 * stride):] = 9
    ends2 = singles.copy()
    ends2[max(0, n_active - 2 * stride):] = 9
    E = 16 // stride
    cuts = keys_of_heads(rng.integers(0, 2, size=(6, 4, stride, E))).transpose(0, 1, 3, 2).reshape(6, 64)
    return np.concatenate([np.stack([one_run, singles, ends, ends2]), cuts]).astype(np.uint32)


def test_lane_runs_partial_waves_stride_1():
    rng = np.random.default_rng(11)
    n_cases = 0
    for n_active in range(1, 65):
        keys = partial_wave_keys(1, n_active, rng)
        assert_lanes(1, keys, lane_values(len(keys), 1), n_active)
        n_cases += len(keys)
    assert n_cases >= 64 * 10                                                 # 64 exec masks x (4 crafted + 6 random) waves


def test_lane_runs_partial_waves_stride_2():
    rng = np.random.default_rng(12)
    n_cases = 0
    for n_active in range(2, 65, 2):
        keys = partial_wave_keys(2, n_active, rng)
        assert_lanes(2, keys, lane_values(len(keys), 2), n_active)
        n_cases += len(keys)
    assert n_cases >= 32 * 10


@pytest.mark.parametrize("stride", (1, 2))
def test_lane_runs_key_all_ones(stride):
    """The header says "any 32-bit key": 0xffffffff is what a lane without a neighbour down the row compares against.  On
    the first lane(s) of a row that key reads as "continues a run", and the run it continues is empty: the contract holds."""
    F = 0xffffffff
    base = (np.arange(64) + 100).astype(np.uint32)
    waves = []
    for n_first in (1, 2, 3, 5, 16):                      # the first lanes of every row, alone and as a run, up to the whole row
        k = base.copy().reshape(4, 16)
        k[:, :n_first * stride if n_first < 16 else 16] = F
        waves.append(k.reshape(64))
    for lo, hi in ((3, 9), (6, 16), (1, 2), (14, 16)):    # inside a row: a run of it in front of, behind and between other keys
        k = base.copy().reshape(4, 16)
        k[:, lo:hi] = F
        waves.append(k.reshape(64))
    k = np.full(64, 5, dtype=np.uint32).reshape(4, 16)    # inside a run of another key
    k[:, 4:6] = F
    waves.append(k.reshape(64))
    keys = np.stack(waves)
    n_runs, _ = assert_lanes(stride, keys, lane_values(len(keys), stride), check_repeat=False)
    assert len(keys) == 10 and n_runs > 10 * 4
    assert_lanes(stride, keys, lane_values(len(keys), stride), n_active=38, check_repeat=False)


@pytest.mark.parametrize("stride", (1, 2))
def test_keys_repeat_counts_the_lanes_that_continue_a_run(stride):
    """keys_repeat is true from 16 lanes that equal their neighbour `stride` down the row: 15, 16 and 17 on full and on
    partial waves."""
    rng = np.random.default_rng(13)
    seen = set()
    for n_active in (64, 40, 22):
        cand = np.array([l for l in range(n_active) if l % 16 >= stride])
        waves = []
        for count in (0, 15, 16, 17, len(cand)):
            for _ in range(3):
                k = (np.arange(64) * 3 + 50).astype(np.uint32)
                for l in np.sort(rng.choice(cand, size=count, replace=False)):
                    k[l] = k[l - stride]
                waves.append(k)
        keys = np.stack(waves)
        _, n_equal = assert_lanes(stride, keys, lane_values(len(keys), stride), n_active)
        seen |= set(n_equal.tolist())
    assert {0, 15, 16, 17} <= seen and max(seen) >= 18


# ------------------------------------------------------------------------------------------------------------------
# kernel level: crafted queues
# ------------------------------------------------------------------------------------------------------------------

def dst_pattern(kind, span, set_len, n_sets, limit, rng):
    """Destinations of one bucket's range.  A trip of a fold's loop takes n_sets register sets of set_len consecutive
    entries; the first set decides keys_repeat for the trip."""
    i = np.arange(span)
    if kind == "distinct":
        d = (i * 7 + 3) % limit
    elif kind == "hot":
        d = np.full(span, limit // 3)
    elif kind == "runs":                                  # sorted runs of 1 .. 40 that restart, as where two tile ranges meet
        out, n = [], 0
        while n < span:
            seg, d0 = int(rng.integers(60, 700)), int(rng.integers(0, max(1, limit // 4)))
            while seg > 0 and d0 < limit:
                ln = int(rng.integers(1, 41))
                out.append(np.full(ln, d0))
                d0 += int(rng.integers(1, 10))
                seg -= ln
                n += ln
        d = np.concatenate(out)[:span] if out else np.zeros(0, dtype=np.int64)
        for p in range(20, span - 4, 256):                # "5 9 | 5 7": equal keys two lanes apart are two runs
            d[p:p + 4] = np.array([5, 9, 5, 7]) % limit
    elif kind in ("mixed_first", "mixed_rest"):           # the trip's first register set repeats, the others do not / the reverse
        first = (i % (set_len * n_sets)) < set_len
        hot = 100 % limit + (i // 16) % min(50, limit)
        d = np.where(first == (kind == "mixed_first"), hot % limit, (i * 7 + 3) % limit)
    elif kind == "straddle":                              # runs of 24 from entry 8 on: across rows of 16, waves of 64 and trips
        d = ((i + 16) // 24 * 5) % limit
    else:
        raise ValueError(kind)
    return d.astype(np.uint16)


PATTERNS = ("distinct", "hot", "runs", "mixed_first", "mixed_rest", "straddle")


def int_values(dst, rng):
    """Integer-valued doubles with zeros among them; the first stretch of equal destinations starts with up to 16 values
    that cancel to 0 (a whole run of a row when the stretch starts one).  Returns the values and how many cancel."""
    v = rng.integers(-40, 41, size=len(dst)).astype(np.float64)
    n_cancel = 0
    if len(dst) >= 2:
        cut = np.flatnonzero(np.diff(dst.astype(np.int64)) != 0) + 1
        start, end = np.concatenate([[0], cut]), np.concatenate([cut, [len(dst)]])
        long = np.flatnonzero(end - start >= 2)
        if len(long):
            s = start[long[0]]
            n_cancel = int(min(end[long[0]] - s, 16) // 2 * 2)
            v[s:s + n_cancel] = np.tile([13.0, -13.0], n_cancel // 2)
    return v, n_cancel


def make_queue(buckets):
    """buckets: a (dst, values [n] or [n, slots]) pair each -> bucket_base, q_dst, queue"""
    base = np.concatenate([[0], np.cumsum([len(d) for d, _ in buckets])]).astype(np.uint32)
    q_dst = np.ascontiguousarray(np.concatenate([d for d, _ in buckets]).astype(np.uint16))
    queue = np.ascontiguousarray(np.concatenate([v for _, v in buckets]).astype(np.float64))
    return base, q_dst, queue


def scatter_reference(base, q_dst, queue, n_txps):
    """(scatter [n_txps(, slots)] by np.add.at, entries per destination, sum |v| per destination)"""
    idx = np.repeat(np.arange(len(base) - 1, dtype=np.int64), np.diff(base.astype(np.int64))) * K_BUCKET + q_dst
    assert len(idx) == 0 or idx.max() < n_txps
    s = np.zeros((n_txps,) + queue.shape[1:])
    a = np.zeros_like(s)
    np.add.at(s, idx, queue)
    np.add.at(a, idx, np.abs(queue))
    return s, np.bincount(idx, minlength=n_txps), a


def initial_counts(shape, touched, rng):
    """Nonzero everywhere: integers where the fold adds, anything where it must not."""
    c = rng.integers(1, 1000, size=shape).astype(np.float64)
    return np.where(touched, c, c + rng.random(size=shape))


def assert_same_bits(got, want, what):
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, f"{what}: {len(bad)} elements differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}"


def remote_fold(base, q_dst, queue, cnt0, n_groups, ntq, threads, done=-1):
    cnt = np.array(cnt0, dtype=np.float64)
    _ok(_lib.testing_lib().oem_test_remote_fold(_p(base), len(base) - 1, _p(queue), _p(q_dst), _p(cnt), len(cnt), n_groups, int(ntq),
                                                threads, done, 0))
    return cnt


FOLD_SPANS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8193)
BIG_GROUPS = 70   # more workgroups per bucket than the spans 0 .. 65 have entries: empty groups


@pytest.mark.parametrize("threads", (1024, 256))
@pytest.mark.parametrize("ntq", (False, True))
def test_remote_fold_is_an_exact_scatter_add(ntq, threads):
    """One bucket per span (a trip is threads x 4 entries), every destination pattern, 1, 2, 3 and 70 workgroups per bucket."""
    rng = np.random.default_rng(100 + threads + int(ntq))
    n_launches = n_cancelled = 0
    for kind in PATTERNS:
        buckets = []
        for span in FOLD_SPANS:
            d = dst_pattern(kind, span, threads, 4, K_BUCKET, rng)
            v, n_cancel = int_values(d, rng)
            buckets.append((d, v))
            n_cancelled += n_cancel
        base, q_dst, queue = make_queue(buckets)
        n_txps = len(buckets) * K_BUCKET
        scatter, n_in, _ = scatter_reference(base, q_dst, queue, n_txps)
        cnt0 = initial_counts(n_txps, n_in > 0, rng)
        want = np.where(n_in > 0, cnt0 + scatter, cnt0)
        for n_groups in (1, 2, 3, BIG_GROUPS):
            got = remote_fold(base, q_dst, queue, cnt0, n_groups, ntq, threads)
            assert_same_bits(got, want, f"k_remote_fold<{ntq}, {threads}> {kind}, {n_groups} groups")
            n_launches += 1
    assert n_launches == len(PATTERNS) * 4 and n_cancelled > 0


def test_remote_fold_last_bucket_is_short_and_done_is_honoured():
    """Two buckets, the second with 17 transcripts: its hot destinations, the flush guard of the last bucket; a run whose
    state says done leaves the counts alone."""
    rng = np.random.default_rng(7)
    n_txps = K_BUCKET + 17
    for kind in ("hot", "runs", "straddle"):
        d0, d1 = dst_pattern(kind, 5000, 1024, 4, K_BUCKET, rng), dst_pattern(kind, 3001, 1024, 4, 17, rng)
        base, q_dst, queue = make_queue([(d0, int_values(d0, rng)[0]), (d1, int_values(d1, rng)[0])])
        scatter, n_in, _ = scatter_reference(base, q_dst, queue, n_txps)
        cnt0 = initial_counts(n_txps, n_in > 0, rng)
        want = np.where(n_in > 0, cnt0 + scatter, cnt0)
        for n_groups in (1, 3):
            assert_same_bits(remote_fold(base, q_dst, queue, cnt0, n_groups, False, 1024, done=0), want, f"{kind}, {n_groups} groups")
        assert_same_bits(remote_fold(base, q_dst, queue, cnt0, 2, True, 256), want, f"{kind}, 256 threads")
        assert_same_bits(remote_fold(base, q_dst, queue, cnt0, 2, False, 1024, done=1), cnt0, f"{kind}, done")


def remote_fold_b(base, q_dst, queue, theta, cnt0, n_groups, phases):
    cnt = np.array(cnt0, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    ph = np.asarray(phases, dtype=np.uint32)
    _ok(_lib.testing_lib().oem_test_remote_fold_b(_p(base), len(base) - 1, _p(queue), _p(q_dst), _p(theta), _p(cnt), cnt.shape[0],
                                                  n_groups, _p(ph), K_BATCH, 0))
    return cnt


FOLD_B_STEP = 8 * 512    # kFoldDepth x entries one load of the workgroup covers
FOLD_B_SPANS = (0, 1, 31, 33, 511, 513, FOLD_B_STEP - 1, FOLD_B_STEP, FOLD_B_STEP + 1, 2 * FOLD_B_STEP - 1, 2 * FOLD_B_STEP, 2 * FOLD_B_STEP + 1)
FOLD_B_PHASES = (RUNNING, FINISHED, FINAL, RUNNING)


def fold_b_reference(scatter, theta, cnt0, phases):
    """cnt[t][slot] += theta * sum for the slots that are not finished; a final slot reads theta < 1e-5 as 0 (em.rs:238-242)"""
    want = cnt0.copy()
    for b, ph in enumerate(phases):
        if ph == FINISHED:
            continue
        th = np.where((ph == FINAL) & (theta[:, b] < MIN_READ_THRESH), 0.0, theta[:, b])
        want[:, b] = cnt0[:, b] + scatter[:, b] * th
    return want


def test_remote_fold_b_is_an_exact_scatter_add():
    """Spans around kStep and 2 kStep of the double-buffered loop; theta is a power of two, so sum * theta is exact; one
    finished slot (nothing of it flushed, whatever its queue holds), one final slot with abundances below the read
    threshold, two running ones."""
    rng = np.random.default_rng(21)
    n_launches = n_small_final = n_cancelled = 0
    for kind in PATTERNS:
        buckets = []
        for span in FOLD_B_SPANS:
            d = dst_pattern(kind, span, 512, 8, K_BUCKET, rng)
            vs = [int_values(d, rng) for _ in range(K_BATCH)]
            buckets.append((d, np.stack([v for v, _ in vs], axis=1).reshape(len(d), K_BATCH)))
            n_cancelled += vs[0][1]
        base, q_dst, queue = make_queue(buckets)
        n_txps = len(buckets) * K_BUCKET - 1000           # (the last bucket is short; its span-8193 range stays below 3096)
        q_dst[base[-2]:] %= K_BUCKET - 1000
        scatter, n_in, _ = scatter_reference(base, q_dst, queue, n_txps)
        theta = 2.0 ** rng.integers(-3, 4, size=(n_txps, K_BATCH))
        theta[rng.random(size=theta.shape) < 0.3] = 2.0 ** -20           # below OEM_MIN_READ_THRESH
        n_small_final += int(((theta[:, 2] < MIN_READ_THRESH) & (scatter[:, 2] != 0.0)).sum())
        cnt0 = initial_counts((n_txps, K_BATCH), (n_in > 0)[:, None], rng)
        want = fold_b_reference(scatter, theta, cnt0, FOLD_B_PHASES)
        assert_same_bits(want[:, 1], cnt0[:, 1], "reference of the finished slot")
        for n_groups in (1, 2, 3):
            got = remote_fold_b(base, q_dst, queue, theta, cnt0, n_groups, FOLD_B_PHASES)
            assert_same_bits(got, want, f"k_remote_fold_b {kind}, {n_groups} groups")
            n_launches += 1
    assert n_launches == len(PATTERNS) * 3 and n_small_final > 100 and n_cancelled > 0
    # every slot finished: the kernel returns before it reads anything
    assert_same_bits(remote_fold_b(base, q_dst, queue, theta, cnt0, 2, (FINISHED,) * K_BATCH), cnt0, "all slots finished")


def multi_fold_reldiff(base, q_dst, queue, theta0, cnt0, out0, T, phases):
    theta, cnt, out = (np.array(a, dtype=np.float64) for a in (theta0, cnt0, out0))
    ph = np.asarray(phases, dtype=np.uint32)
    rel = np.zeros(len(ph), dtype=np.uint64)
    _ok(_lib.testing_lib().oem_test_multi_fold_reldiff(_p(base), len(base) - 1, _p(queue), _p(q_dst), _p(theta), _p(cnt), _p(out),
                                                       len(theta), T, _p(ph), _p(rel), 0))
    return theta, cnt, out, rel


def multi_reference(scatter, theta0, cnt0, out0, T, phases):
    """em.rs:204-207 and :254 per element, from the exact cnt + scatter; a bucket whose cells are all finished is skipped,
    a finished cell's elements are left alone; rel_bits = the cell's maximum of rel_diff_term (em.rs:194-201)."""
    n_txps = len(theta0)
    ph = np.asarray(phases)[np.arange(n_txps) // T]
    upd = ph != FINISHED
    cc = cnt0 + scatter
    cnt = np.where(upd, 0.0, cnt0)
    out = np.where(upd & (ph == FINAL), cc, out0)
    theta = np.where(upd & (ph == RUNNING), cc, theta0)
    with np.errstate(divide="ignore", invalid="ignore"):
        term = np.where(upd & (ph == RUNNING) & (theta0 > MIN_READ_THRESH), (cc - theta0) / theta0, 0.0)
    rel = np.zeros(len(phases))
    np.maximum.at(rel, np.arange(n_txps) // T, np.maximum(term, 0.0))
    return theta, cnt, out, rel.view(np.uint64)


@pytest.mark.parametrize("T,n_cells,phase_sets", [
    (1500, 3, ((RUNNING, FINAL, FINISHED), (FINISHED, RUNNING, RUNNING), (FINAL, FINISHED, FINAL), (FINISHED,) * 3)),
    (50, 100, (None,)),
])
def test_multi_fold_reldiff_is_an_exact_scatter_add_and_sweep(T, n_cells, phase_sets):
    """T = 1500: bucket 0 is shared by three cells, bucket 1 holds the rest of the third (404 transcripts: a short window,
    and a bucket that is skipped when that cell is finished).  T = 50: 82 cells in bucket 0, more than the 64 whose maxima
    are kept in the LDS."""
    rng = np.random.default_rng(31 + T)
    n_txps = T * n_cells
    n_buckets = (n_txps + K_BUCKET - 1) // K_BUCKET
    n_checked = 0
    for kind in PATTERNS:
        buckets = []
        for b, span in zip(range(n_buckets), (4097 + 1024 + 65, 1025)):
            d = dst_pattern(kind, span, 1024, 4, min(K_BUCKET, n_txps - b * K_BUCKET), rng)
            buckets.append((d, int_values(d, rng)[0]))
        base, q_dst, queue = make_queue(buckets)
        scatter, n_in, _ = scatter_reference(base, q_dst, queue, n_txps)
        cnt0 = initial_counts(n_txps, True, rng)
        theta0 = 2.0 ** rng.integers(-4, 5, size=n_txps)                  # powers of two: (cc - pc) / pc is exact
        theta0[rng.random(size=n_txps) < 0.2] = 2.0 ** -20                # at or below the read threshold: no term
        out0 = rng.random(size=n_txps) + 1.0
        for phases in phase_sets:
            if phases is None:
                phases = rng.integers(0, 3, size=n_cells)
            got = multi_fold_reldiff(base, q_dst, queue, theta0, cnt0, out0, T, phases)
            want = multi_reference(scatter, theta0, cnt0, out0, T, phases)
            for g, w, name in zip(got[:3], want[:3], ("theta", "cnt", "out")):
                assert_same_bits(g, w, f"k_multi_fold_reldiff T={T} {kind} phases {list(phases)[:8]}: {name}")
            assert got[3].tolist() == want[3].tolist(), (T, kind, list(phases)[:8])
            n_checked += int((want[3] != 0).sum())
    assert n_checked >= len(PATTERNS)                                     # nonzero maxima were compared, not only zeros


def test_folds_on_lognormal_values_stay_inside_the_reordering_bound():
    """Values that round: each destination within (n - 1) 2^-53 sum|v| of the float64 add.at, n entries summed into it --
    the worst case of any order of summation, from zero counts."""
    rng = np.random.default_rng(41)
    n_txps = 2 * K_BUCKET
    n_checked = 0
    for kind in ("runs", "hot", "straddle"):
        buckets = []
        for span in (4097, 1500):
            d = dst_pattern(kind, span, 1024, 4, K_BUCKET, rng)
            buckets.append((d, rng.lognormal(0.0, 2.0, size=(len(d), K_BATCH))))
        base, q_dst, queue4 = make_queue(buckets)
        queue = np.ascontiguousarray(queue4[:, 0])
        scatter, n_in, sum_abs = scatter_reference(base, q_dst, queue, n_txps)
        bound = np.maximum(n_in - 1, 0) * U * sum_abs
        zero = np.zeros(n_txps)
        for n_groups, ntq, threads in ((1, False, 1024), (3, True, 1024), (2, False, 256)):
            got = remote_fold(base, q_dst, queue, zero, n_groups, ntq, threads)
            assert np.all(np.abs(got - scatter) <= bound), (kind, n_groups, float(np.max(np.abs(got - scatter) - bound)))
        theta, cnt, out, _ = multi_fold_reldiff(base, q_dst, queue, np.ones(n_txps), zero, zero, K_BUCKET, (RUNNING, FINAL))
        assert np.all(np.abs(theta[:K_BUCKET] - scatter[:K_BUCKET]) <= bound[:K_BUCKET]), kind
        assert np.all(np.abs(out[K_BUCKET:] - scatter[K_BUCKET:]) <= bound[K_BUCKET:]) and not cnt.any(), kind
        scatter4, _, sum_abs4 = scatter_reference(base, q_dst, queue4, n_txps)
        theta4 = 2.0 ** rng.integers(-3, 4, size=(n_txps, K_BATCH))
        got4 = remote_fold_b(base, q_dst, queue4, theta4, np.zeros((n_txps, K_BATCH)), 2, (RUNNING,) * K_BATCH)
        bound4 = np.maximum(n_in - 1, 0)[:, None] * U * sum_abs4 * theta4
        assert np.all(np.abs(got4 - scatter4 * theta4) <= bound4), kind
        n_checked += int((n_in > 1).sum())
    assert n_checked > 300                                                # destinations with more than one entry: a real bound
