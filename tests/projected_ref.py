"""Plain-Python restatement of AlignmentFilters::filter_projected and add_projected_group (TEST INFRASTRUCTURE ONLY), and
the inputs the projected-filter tests share: packing, the edge list, seeded random groups.

Reference: src/util/oarfish_types.rs:1179-1297 (filter_projected), :1142-1164 (ProjectedAlnRecord), :695-715
(add_projected_group), :718-738 (add_filtered_group), src/prog_opts.rs:48-57 (ProjProbSource).  Written record by record
with Python loops, independently of oarfish_amd/csrc/oem_filter_projected.h; f32 arithmetic through numpy.float32 and the
C library's expf (what Rust's f32::exp lowers to), as oracle/filter_py.py does it.
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from oarfish_amd import _lib
from oarfish_amd.builder import PROJ_RECORD, StoreBuilder
from oracle import filter_py as fp

f32 = np.float32
F64_MIN = -1.7976931348623157e308
I32_MIN = -2 ** 31
SOURCES = ("similarity", "score", "combined")


@dataclass
class PRec:
    ref_id: int
    start: int
    end: int
    aligned_len: int
    query_aligned_len: int
    similarity: float
    aln_score: int = 0
    reverse: bool = False


def _wrap_i32(v):
    return ((v + 2 ** 31) % 2 ** 32) - 2 ** 31


def libm_expf(x):
    return f32(fp._libm.expf(ctypes.c_float(float(x))))


def filter_projected(dt, F, txp_len, recs, read_len, beta, source):
    """-> [(ref_id, start, end, strand, f)] of the kept records; dt is updated.  A ref_id outside the transcripts or a
    transcript of length 0 -- where the reference would panic -- raises IndexError(record index) before dt is touched."""
    for i, r in enumerate(recs):
        if r.ref_id >= len(txp_len) or int(txp_len[r.ref_id]) == 0:
            raise IndexError(i)
    best_sim, best_score, frac_best = F64_MIN, I32_MIN, f32(0)          # :1188-1190
    kept = []
    for r in recs:                                                      # :1193-1238
        if (F.which_strand == 2 and not r.reverse) or (F.which_strand == 1 and r.reverse):
            dt["discard_ori"] += 1; continue                            # :1199-1202
        if r.aligned_len < F.min_aligned_len:
            dt["discard_aln_len"] += 1; continue                        # :1206-1209
        if r.end <= int(txp_len[r.ref_id]) - F.three_prime_clip:
            dt["discard_3p"] += 1; continue                             # :1214-1217
        if r.start >= F.five_prime_clip:
            dt["discard_5p"] += 1; continue                             # :1220-1223
        if r.similarity > best_sim:                                     # :1226-1233 (False for a NaN)
            best_sim = r.similarity
            frac_best = f32(r.query_aligned_len) / f32(read_len) if read_len > 0 else f32(0)
        if r.aln_score > best_score:                                    # :1234-1236
            best_score = r.aln_score
        kept.append(r)
    if not kept or best_sim <= 0.0:                                     # :1240-1242
        return []
    if frac_best < f32(F.min_aligned_fraction):                         # :1243-1246
        dt["discard_aln_frac"] += 1
        return []
    dt["valid_best_aln"] += 1                                           # :1248
    inv_msim = np.float64(1.0) / np.float64(best_sim)                   # :1251
    out = []
    D, B = f32(F.score_prob_denom), f32(beta)
    with np.errstate(all="ignore"):
        for r in kept:                                                  # :1255-1294
            if not (f32(np.float64(r.similarity) * inv_msim) >= f32(F.score_threshold)):
                dt["discard_score"] += 1; continue                      # :1256-1260
            tlen = int(txp_len[r.ref_id]) % 2 ** 32                     # `as u32` (:1265)
            start = min(max(r.start, 1), tlen)                          # :1266
            end = min(max(r.end, start), tlen)                          # :1267
            by_sim = f32(np.float64(r.similarity) - np.float64(best_sim))
            by_score = f32(_wrap_i32(r.aln_score - best_score)) / D
            if source == "similarity":
                f = by_sim * B                                          # :1275
            elif source == "score":
                f = by_score                                            # :1276
            else:
                f = by_score + B * by_sim                               # :1278-1279
            out.append((r.ref_id, start, end, 1 if r.reverse else 0, f32(f)))
    return out


def add_projected_group(st: fp.Store, F, txp_len, recs, read_len, beta=10.0, source="similarity"):
    """:695-715 on an oracle Store; returns the number of alignments appended"""
    if not recs:                                                        # :703-705
        return 0
    alns = filter_projected(st.dt, F, txp_len, recs, read_len, beta, source)
    for ref_id, start, end, strand, f in alns:                          # :1282-1293
        st.as_prob.append(libm_expf(f))
        st.tid.append(ref_id); st.start.append(start); st.end.append(end); st.strand.append(strand)
    if alns:
        st.row_ptr.append(len(st.tid))                                  # :733
    return len(alns)


def oracle_state(st: fp.Store):
    """an oracle Store as tests.filter_common.state gives a builder"""
    arrs = (np.asarray(st.row_ptr, dtype=np.uint64), np.asarray(st.tid, dtype=np.uint32), np.asarray(st.as_prob, dtype=np.float32),
            np.asarray(st.start, dtype=np.uint32), np.asarray(st.end, dtype=np.uint32), np.asarray(st.strand, dtype=np.uint8))
    return tuple(a.tobytes() for a in arrs) + ((len(st.row_ptr) - 1, len(st.tid)), tuple(sorted(st.dt.items())))


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def pack(groups, read_lens):
    """list of lists of PRec, list of read lengths -> (records, group_off, read_len)"""
    rec = np.zeros(sum(len(g) for g in groups), dtype=PROJ_RECORD)
    off = np.zeros(len(groups) + 1, dtype=np.uint64)
    i = 0
    for k, g in enumerate(groups):
        for x in g:
            rec[i] = (x.similarity, x.ref_id, x.start, x.end, x.aligned_len, x.query_aligned_len, x.aln_score,
                      _lib.REC_REVERSE if x.reverse else 0, 0)
            i += 1
        off[k + 1] = i
    return rec, off, np.asarray(read_lens, dtype=np.uint64)


def random_groups(seed, n_groups, T=50, max_records=13):
    """(F, txp_len, groups, read_lens): groups of 0 .. max_records - 1 records around a best similarity, with the odd
    NaN, non-positive best, zero read length and out-of-range coordinate"""
    from tests.filter_common import random_filters
    rng = np.random.default_rng([seed, 0x9207])
    txp_len = rng.integers(300, 4000, size=T)
    F = random_filters(rng)
    groups, read_lens = [], []
    for _ in range(n_groups):
        n = int(rng.integers(0, max_records))
        read_len = 0 if rng.random() < 0.02 else int(rng.integers(200, 3000))
        best = float(rng.random() * 0.6 + 0.4) if rng.random() > 0.04 else float(rng.random() - 1.0)
        best_score = int(rng.integers(-50, 4000))
        g = []
        for _j in range(n):
            t = int(rng.integers(0, T))
            L = int(txp_len[t])
            span = int(rng.integers(20, 3000))
            start = int(rng.integers(0, 450 if rng.random() < 0.8 else L))
            end = start + span if rng.random() < 0.2 else min(start + span, L)
            u = rng.random()
            sim = best if u < 0.25 else (float("nan") if u < 0.28 else best - float(rng.random()) * (0.12 if u < 0.8 else 1.5))
            g.append(PRec(t, start, end, span, int(rng.integers(0, max(1, read_len) + 1)), sim,
                          best_score - int(rng.integers(0, 40)), reverse=rng.random() < 0.3))
        groups.append(g)
        read_lens.append(read_len)
    return F, txp_len, groups, read_lens


def edge_groups():
    """(name, filters, txp_len, group, read_len) of the edge list; shared with the GPU tests"""
    D = fp.Filters()
    L = [2000] * 8
    ok = lambda t, sim, sc=100, **kw: PRec(t, 10, 1500, 1400, 1400, sim, sc, **kw)      # noqa: E731
    out = [
        ("empty", D, L, [], 1500),
        ("one", D, L, [ok(0, 0.9)], 1500),
        ("ori forward only", fp.Filters(which_strand=1), L, [ok(0, 0.95, reverse=True), ok(1, 0.9)], 1500),
        ("ori reverse only", fp.Filters(which_strand=2), L, [ok(0, 0.95), ok(1, 0.9, reverse=True)], 1500),
        ("aln_len", D, L, [PRec(0, 10, 59, 49, 1400, 0.95), ok(1, 0.9)], 1500),
        ("3p", fp.Filters(three_prime_clip=600), L, [PRec(0, 10, 1400, 1390, 1400, 0.95), PRec(1, 10, 1401, 1391, 1400, 0.9)], 1500),
        ("5p", fp.Filters(five_prime_clip=400), L, [PRec(0, 400, 1800, 1400, 1400, 0.95), PRec(1, 399, 1800, 1401, 1400, 0.9)], 1500),
        ("score", D, L, [ok(0, 1.0), ok(1, 0.9499), ok(2, 0.9501)], 1500),
        ("aln_frac", D, L, [PRec(0, 10, 1500, 1400, 749, 0.95), ok(1, 0.9)], 1500),
        ("tie: the first decides the fraction", D, L, [PRec(0, 10, 1500, 1400, 700, 0.9), ok(1, 0.9)], 1500),
        ("tie: the first decides the fraction (kept)", D, L, [ok(0, 0.9), PRec(1, 10, 1500, 1400, 700, 0.9)], 1500),
        ("best score and best similarity apart", fp.Filters(score_threshold=0.5), L, [ok(0, 0.9, 50), ok(1, 0.7, 80), ok(2, 0.8, 20)], 1500),
        ("best similarity 0", D, L, [ok(0, 0.0), ok(1, -0.5)], 1500),
        ("best similarity negative", D, L, [ok(0, -0.25), ok(1, -0.5)], 1500),
        ("nan similarity", D, L, [ok(0, float("nan")), ok(1, 0.9), ok(2, float("nan"))], 1500),
        ("nan only", D, L, [ok(0, float("nan"))], 1500),
        ("read_len 0", D, L, [ok(0, 0.9)], 0),
        ("read_len 0, fraction 0 allowed", fp.Filters(min_aligned_fraction=0.0), L, [ok(0, 0.9)], 0),
        ("threshold 1.5", fp.Filters(score_threshold=1.5), L, [ok(0, 0.9), ok(1, 0.9)], 1500),
        ("start 0 and end beyond the transcript", D, L, [PRec(0, 0, 2500, 2500, 1400, 0.9), PRec(1, 2100, 2600, 500, 1400, 0.89)], 1500),
        ("score difference wraps", fp.Filters(score_threshold=0.0), L, [ok(0, 0.9, 2 ** 31 - 1), ok(1, 0.8, -2 ** 31)], 1500),
        ("huge similarities", fp.Filters(score_threshold=-1.0), L, [ok(0, 1e308), ok(1, -1e308), ok(2, 5e307)], 1500),
        ("5p at u32 max", fp.Filters(five_prime_clip=2 ** 32 - 1), L, [PRec(0, 2 ** 32 - 1, 2 ** 32 - 1, 1400, 1400, 0.95), ok(1, 0.9)], 1500),
    ]
    for n in (63, 64, 65, 300):
        out.append((f"{n} records", D, L, [ok(j % 8, 0.99 - (j % 97) * 1e-3, 500 - j % 31, reverse=j % 3 == 0) for j in range(n)], 1500))
    return out


def host_loop(F, txp_len, groups, read_lens, beta, source, into: StoreBuilder = None):
    """the add_projected_group loop; returns (builder, kept)"""
    from tests.filter_common import filters_dict
    b = into if into is not None else StoreBuilder(filters_dict(F), txp_len)
    kept = np.zeros(len(groups), dtype=np.uint32)
    for k, (g, rl) in enumerate(zip(groups, read_lens)):
        kept[k] = b.add_projected_group(pack([g], [rl])[0], rl, beta=beta, prob_source=source)
    return b, kept


def oracle_loop(F, txp_len, groups, read_lens, beta, source, into: fp.Store = None):
    ref = into if into is not None else fp.Store()
    kept = np.array([add_projected_group(ref, F, txp_len, g, rl, beta, source) for g, rl in zip(groups, read_lens)], dtype=np.uint32)
    return ref, kept


def last_projected_pass(L):
    """What the test-only library L recorded of this thread's last projected device batch call: (k_proj_measure ms,
    k_proj_emit ms, host finish ms, alignments finished by the host, alignments emitted)."""
    out = (ctypes.c_double * 5)()
    assert L.oem_debug_proj_last_pass(out) == 0
    return float(out[0]), float(out[1]), float(out[2]), int(out[3]), int(out[4])
