"""Shared helpers of tests/test_filter_groups.py and tests/test_filter_groups_gpu.py: record groups as the batch calls
take them, the seeded random groups of tests/test_builder.py's recipe, and a builder's whole visible state."""
import ctypes
import dataclasses

import numpy as np

from oarfish_amd import _lib
from oarfish_amd.builder import ALN_RECORD, StoreBuilder
from oracle import filter_py as fp


def filters_dict(F: fp.Filters) -> dict:
    return dataclasses.asdict(F)


def pack(groups):
    """list of lists of fp.Rec -> (records, group_off)"""
    n = sum(len(g) for g in groups)
    rec = np.zeros(n, dtype=ALN_RECORD)
    off = np.zeros(len(groups) + 1, dtype=np.uint64)
    i = 0
    for k, g in enumerate(groups):
        for x in g:
            flags = (_lib.REC_UNMAPPED if x.unmapped else 0) | (_lib.REC_REVERSE if x.reverse else 0) | \
                    (_lib.REC_SUPPLEMENTARY if x.supp else 0) | (_lib.REC_HAS_SCORE if x.score is not None else 0)
            rec[i] = (x.ref_id, x.aln_start, x.aln_end, x.aln_span, x.score if x.score is not None else 0,
                      x.seq_len if x.seq_len is not None else -1, flags, 0)
            i += 1
        off[k + 1] = i
    return rec, off


def random_filters(rng) -> fp.Filters:
    return fp.Filters(five_prime_clip=int(rng.choice([2 ** 32 - 1, 400])), three_prime_clip=int(rng.choice([2 ** 62, 600])),
                      score_threshold=float(rng.choice([0.95, 0.9])), min_aligned_fraction=float(rng.choice([0.5, 0.7])),
                      min_aligned_len=int(rng.choice([50, 200])), which_strand=int(rng.integers(0, 3)),
                      score_prob_denom=float(rng.choice([5.0, 2.5])))


def random_groups(seed, n_groups, T=50, max_records=7):
    """(F, txp_len, groups): the generator of tests/test_builder.py::_builder_matches_python_restatement"""
    rng = np.random.default_rng(seed)
    txp_len = rng.integers(300, 4000, size=T)
    F = random_filters(rng)
    groups = []
    for _ in range(n_groups):
        n = int(rng.integers(0, max_records))
        read_len = int(rng.integers(200, 3000))
        best = int(rng.integers(-5, 3000))
        g = []
        for j in range(n):
            t = int(rng.integers(0, T))
            span = int(rng.integers(20, read_len + 1))
            start = int(rng.integers(0, max(1, int(txp_len[t]) - 10)))
            sc = None if rng.random() < 0.03 else int(best - rng.integers(0, max(1, abs(best) // 8 + 2)))
            g.append(fp.Rec(t, start, start + span, span, sc, read_len if (j == 0 or rng.random() < 0.5) else None,
                            unmapped=rng.random() < 0.05, reverse=rng.random() < 0.3, supp=rng.random() < 0.05))
        groups.append(g)
    return F, txp_len, groups


def state(b: StoreBuilder):
    """everything oem_builder_export, _dims and _discard_table show, as bytes"""
    return tuple(a.tobytes() for a in b.export()) + (b.dims(), tuple(sorted(b.discard_table().items())))


def host_loop(F, txp_len, groups, into: StoreBuilder = None):
    """the add_group loop; returns (builder, kept)"""
    b = into if into is not None else StoreBuilder(filters_dict(F), txp_len)
    kept = np.zeros(len(groups), dtype=np.uint32)
    for k, g in enumerate(groups):
        rec, _ = pack([g])
        kept[k] = b.add_group(rec)
    return b, kept


def oracle_loop(F, txp_len, groups):
    ref = fp.Store()
    kept = np.array([fp.add_group(ref, F, txp_len, g) for g in groups], dtype=np.uint32)
    return ref, kept


def f32_bits(x: float) -> int:
    return int(np.float32(x).view(np.uint32))


def libm_expf(x):
    return np.float32(fp._libm.expf(ctypes.c_float(float(x))))


def edge_groups():
    """(name, filters, txp_len, group) of the edge list; shared with the GPU tests"""
    D = fp.Filters()
    L = [2000] * 8
    ok = lambda t, sc, **kw: fp.Rec(t, 10, 1500, 1400, sc, 1500, **kw)      # noqa: E731
    out = [
        ("empty", D, L, []),
        ("one", D, L, [ok(0, 1000)]),
        ("unmapped only", D, L, [fp.Rec(0, 0, 0, 0, None, 100, unmapped=True), fp.Rec(2 ** 32 - 1, 0, 0, 0, 5, None, unmapped=True)]),
        ("non-positive best", D, L, [ok(0, 0), ok(1, -7)]),
        ("zero span at best", D, L, [fp.Rec(0, 10, 10, 0, 1000, 1500), ok(1, 990)]),
        ("ori forward only", fp.Filters(which_strand=1), L, [ok(0, 1000, reverse=True), ok(1, 900)]),
        ("ori reverse only", fp.Filters(which_strand=2), L, [ok(0, 1000), ok(1, 900, reverse=True)]),
        ("supp", D, L, [ok(0, 1000, supp=True), ok(1, 900)]),
        ("aln_len", D, L, [fp.Rec(0, 10, 59, 49, 1000, 1500), ok(1, 900)]),
        ("3p", fp.Filters(three_prime_clip=600), L, [fp.Rec(0, 10, 1400, 1390, 1000, 1500), fp.Rec(1, 10, 1401, 1391, 900, None)]),
        ("5p", fp.Filters(five_prime_clip=400), L, [fp.Rec(0, 400, 1800, 1400, 1000, 1500), fp.Rec(1, 399, 1800, 1401, 900, None)]),
        ("score", D, L, [ok(0, 1000), ok(1, 949), ok(2, 950)]),
        ("aln_frac", D, L, [fp.Rec(0, 10, 759, 749, 1000, 1500), ok(1, 990)]),
        ("tie: the first decides the fraction", D, L, [fp.Rec(0, 10, 710, 700, 1000, 1500), fp.Rec(1, 10, 1500, 1490, 1000, None)]),
        ("tie: the first decides the fraction (kept)", D, L, [fp.Rec(0, 10, 1500, 1490, 1000, 1500), fp.Rec(1, 10, 710, 700, 1000, None)]),
        ("no score, threshold 0", fp.Filters(score_threshold=0.0), L, [ok(0, 700), ok(1, None)]),
        ("no score, threshold -1", fp.Filters(score_threshold=-1.0), L, [ok(0, 700), ok(1, None), ok(2, -300)]),
        ("no score, default threshold", D, L, [ok(0, 700), ok(1, None)]),
        ("seq_len on the third record", D, L, [fp.Rec(0, 10, 1500, 1400, 1000, None), fp.Rec(1, 10, 1500, 1400, 990, None), fp.Rec(2, 10, 1500, 1400, 980, 2000)]),
        ("no seq_len at all", D, L, [fp.Rec(0, 10, 1500, 1400, 1000, None)]),
        ("threshold 1.5", fp.Filters(score_threshold=1.5), L, [ok(0, 1000), ok(1, 1000)]),
        ("table end", fp.Filters(score_threshold=-1.0), L, [ok(0, 600), ok(1, 600 - 519), ok(2, 600 - 520), ok(3, 600 - 521), ok(4, -500)]),
        ("clips at their defaults' extremes", fp.Filters(three_prime_clip=2 ** 62, five_prime_clip=2 ** 32 - 1), L, [fp.Rec(0, 2 ** 32 - 2, 2 ** 32 - 1, 1400, 1000, 1500)]),
        ("5p at u32 max", fp.Filters(five_prime_clip=2 ** 32 - 1), L, [fp.Rec(0, 2 ** 32 - 1, 2 ** 32 - 1, 1400, 1000, 1500), ok(1, 1000)]),
        ("score wraps as i32", D, L, [ok(0, 2 ** 32 + 1000), ok(1, 990)]),
    ]
    for n in (63, 64, 65, 300):
        out.append((f"{n} records", D, L, [ok(j % 8, 2000 - (j % 97), reverse=j % 3 == 0, supp=j % 41 == 40) for j in range(n)]))
    return out


def last_device_pass(L):
    """What the test-only library L timed of this thread's last device batch call under OEM_FILTER_TIMING=1:
    (k_filter_measure ms, k_filter_emit ms); zeros where that kernel did not run."""
    ms = (ctypes.c_float * 6)()
    assert L.oem_debug_filter_last_timing(ms) == 0
    return float(ms[1]), float(ms[3])
