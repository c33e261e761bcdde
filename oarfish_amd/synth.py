"""Seeded synthetic alignment stores for the BASELINE.json configurations.

Generator of SURVEY.md section 8d / BASELINE.md section 4 (there is no BAM or
read data in the reference's test_data/, and no network):

  * true abundance  a_t ~ LogNormal(0, 2), normalised;
  * transcripts grouped into "genes" of size 1 + Geom(1/4), contiguous ids;
  * per read: primary t0 ~ Categorical(a); k = clip(1 + Poisson(kbar-1), 1, 100)
    (cap = --best-n default 100, prog_opts.rs:428); the other k-1 targets are 80 %
    from the primary's gene and 20 % uniform over all transcripts; duplicates within
    a read are dropped (targets are distinct);
  * weights follow oarfish_types.rs:1107-1113: p = expf((s - best) / 5) as **f32**,
    with d = best - s in {0, 1, ...}: d = 0 for the primary, d ~ Geom(0.15) for the
    others, truncated so that s / best >= 0.95 (default score threshold,
    prog_opts.rs:458) for a best score drawn uniformly from [500, 3000];
  * optional coverage column: positive f64, normalised to sum 1 per read, as
    normalize_probability.rs:61-69 leaves it.

Rows come out in generation order (no sorting).  Reads are generated in fixed
chunks of ``CHUNK`` reads, chunk c from ``default_rng([seed, c])``, so a store is
a pure function of (seed, n_reads, n_txps, kbar, coverage).
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Optional

import numpy as np

CHUNK = 1 << 18
BASE_SEED = 20260928


@dataclass
class SyntheticStore:
    row_ptr: np.ndarray          # u64 [R+1]
    tid: np.ndarray              # u32 [nnz]
    as_prob: np.ndarray          # f32 [nnz]
    cov_prob: Optional[np.ndarray]  # f64 [nnz] or None
    n_txps: int
    abundance: np.ndarray        # f64 [T] ground truth (sums to 1)
    gene_of: np.ndarray          # i32 [T]

    @property
    def n_reads(self) -> int:
        return len(self.row_ptr) - 1

    @property
    def nnz(self) -> int:
        return len(self.tid)


def _genes(n_txps: int, rng: np.random.Generator):
    sizes = []
    tot = 0
    while tot < n_txps:
        s = 1 + rng.geometric(0.25, size=max(1024, n_txps // 3)) - 1  # 1 + Geom(1/4) on {0,1,..}
        sizes.append(s)
        tot += int(s.sum())
    sizes = np.concatenate(sizes)
    ends = np.cumsum(sizes)
    n_genes = int(np.searchsorted(ends, n_txps, side="left")) + 1
    sizes = sizes[:n_genes].copy()
    sizes[-1] -= int(ends[n_genes - 1]) - n_txps
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    gene_of = np.repeat(np.arange(n_genes, dtype=np.int32), sizes)
    return starts, sizes.astype(np.int64), gene_of


def _families(n_genes: int, rng: np.random.Generator, adjacent: bool):
    """Paralog families of three genes: consecutive triples of a random permutation of the genes (scattered over the
    annotation, as an annotation numbers them), or of the genes in id order (``adjacent``: the numbering a co-mapping
    renumbering at store creation would produce).  Returns (order, pos): family f = order[3 f : 3 f + 3], pos = inverse."""
    order = np.arange(n_genes, dtype=np.int64) if adjacent else rng.permutation(n_genes).astype(np.int64)
    pos = np.empty(n_genes, dtype=np.int64)
    pos[order] = np.arange(n_genes, dtype=np.int64)
    return order, pos


def _chunk(c: int, n: int, seed: int, n_txps: int, kbar: float, cdf, g_start, g_size, gene_of,
           coverage: bool, gaps: str = "geometric", fam=None):
    rng = np.random.default_rng([seed, c])
    # primary transcript ~ Categorical(a)
    t0 = np.searchsorted(cdf, rng.random(n), side="right").astype(np.int64)
    np.minimum(t0, n_txps - 1, out=t0)
    k = np.clip(1 + rng.poisson(max(kbar - 1.0, 0.0), size=n), 1, 100).astype(np.int64)
    k = np.minimum(k, n_txps)
    tot = int(k.sum())
    row = np.repeat(np.arange(n, dtype=np.int64), k)
    first = np.concatenate([[0], np.cumsum(k)[:-1]])
    is_primary = np.zeros(tot, dtype=bool)
    is_primary[first] = True
    # targets: slot 0 is the primary; of the other k-1 slots Binomial(k-1, 0.8) are
    # "same gene" slots, the rest uniform over all transcripts.  Same-gene slots walk
    # the gene's other members from a random rotation (distinct by construction) and,
    # once the gene is exhausted, spill to the ids that follow it (neighbouring
    # genes), so reads keep their k alignments and their locality.
    slot = np.arange(tot, dtype=np.int64) - first[row]
    n_gene = rng.binomial(k - 1, 0.8)[row]
    is_gene = (slot >= 1) & (slot <= n_gene)
    g = gene_of[t0][row]
    gs, gz = g_start[g], g_size[g]
    i = slot - 1
    rot = (rng.random(n) * 1e9).astype(np.int64)[row]
    others = np.maximum(gz - 1, 1)
    member = (t0[row] - gs + 1 + (rot + i) % others) % gz
    spill = gs + gz + (i - (gz - 1))
    spill = np.where(spill >= n_txps, gs - 1 - (spill - n_txps), spill)
    in_gene = np.where(i < gz - 1, gs + member, spill)
    in_gene = np.clip(in_gene, 0, n_txps - 1)
    if fam is None:
        anywhere = rng.integers(0, n_txps, size=tot)
    else:
        # far hits recur: a transcript of another gene of the read's paralog family (three genes), not anywhere
        order, pos = fam
        n_genes = len(order)
        ps = pos[g]
        # (the last family is incomplete when the gene count is no multiple of three: the index wraps inside the family's
        # real size, so its reads still draw their far hit from ANOTHER gene -- a family of one has only itself)
        fsize = np.minimum(3, n_genes - 3 * (ps // 3))
        step = np.where(fsize == 3, 1 + rng.integers(0, 2, size=tot), 1)
        other = 3 * (ps // 3) + (ps % 3 + step) % fsize
        g2 = order[other]
        anywhere = g_start[g2] + (rng.random(tot) * g_size[g2]).astype(np.int64)
    t = np.where(is_gene, in_gene, anywhere)
    t[is_primary] = t0
    # score deficits d (best - s): 0 for the primary, truncated geometric otherwise
    if gaps == "uniform":
        # Long reads: a best score anywhere in [500, 20 000] and the other alignments' deficits UNIFORM on everything
        # the reference's score_threshold of 0.95 lets through (oarfish_types.rs:1107-1118) -- up to 1000 distinct
        # integer gaps, of which exp(-gap / 5) keeps ~520 apart in f32 before it reaches 0: the store with more than
        # 256 distinct weights that the byte-coded weight table cannot take (oem_layout_dict.hip: 16-bit indices).
        best = rng.integers(500, 20001, size=n)
        dmax = np.floor(0.05 * best).astype(np.int64)[row]
        d = np.floor(rng.random(tot) * (dmax + 1)).astype(np.int64)
    else:
        best = rng.integers(500, 3001, size=n)
        dmax = np.floor(0.05 * best).astype(np.int64)[row]
        d = np.minimum(rng.geometric(0.15, size=tot) - 1, dmax)
    d[is_primary] = 0
    # distinct targets per read: keep the smallest deficit of each (row, tid)
    order = np.lexsort((d, t, row))
    row, t, d = row[order], t[order], d[order]
    keep = np.ones(tot, dtype=bool)
    keep[1:] = (row[1:] != row[:-1]) | (t[1:] != t[:-1])
    row, t, d = row[keep], t[keep], d[keep]
    # oarfish_types.rs:1112-1113: ((fscore - mscore) / score_prob_denom).exp() in f32
    p = np.exp((-d.astype(np.float32)) / np.float32(5.0)).astype(np.float32)
    lens = np.bincount(row, minlength=n).astype(np.uint64)
    cov = None
    if coverage:
        cov = rng.uniform(0.05, 1.0, size=len(t))
        s = np.add.reduceat(cov, np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64))
        cov = cov / np.repeat(s, lens.astype(np.int64))
    return lens, t.astype(np.uint32), p, cov


def make_store(n_reads: int, n_txps: int, kbar: float = 8.0, seed: int = BASE_SEED,
               coverage: bool = False, threads: int = 8, gaps: str = "geometric", far: str = "uniform") -> SyntheticStore:
    """``gaps``: "geometric" (score deficits Geom(0.15), best score 500..3000 -- ~100 distinct
    weights) or "uniform" (long reads: deficits uniform on [0, 0.05 best], best score 500..20 000 -- ~520 distinct
    weights; see _chunk).
    ``far``: where a read's alignments outside its gene go (20 % of the non-primary ones): "uniform" -- anywhere in the
    annotation, SURVEY.md section 8d's generator and the BASELINE headline; "paralog" -- a transcript of another gene of
    the read's paralog FAMILY (three genes scattered over the annotation): far hits recur, as multi-mapping reads'
    do; "paralog_adjacent" -- the same families numbered next to each other (the annotation a co-mapping renumbering
    of the transcripts at store creation would produce)."""
    if gaps not in ("geometric", "uniform"):
        raise ValueError("gaps must be 'geometric' or 'uniform'")
    if far not in ("uniform", "paralog", "paralog_adjacent"):
        raise ValueError("far must be 'uniform', 'paralog' or 'paralog_adjacent'")
    rng0 = np.random.default_rng([seed, 0xA11CE])
    a = rng0.lognormal(0.0, 2.0, size=n_txps)
    a /= a.sum()
    cdf = np.cumsum(a)
    cdf /= cdf[-1]
    g_start, g_size, gene_of = _genes(n_txps, rng0)
    fam = None if far == "uniform" else _families(len(g_start), np.random.default_rng([seed, 0xFA111E5]), far == "paralog_adjacent")
    n_chunks = (n_reads + CHUNK - 1) // CHUNK
    sizes = [min(CHUNK, n_reads - c * CHUNK) for c in range(n_chunks)]

    def run(c):
        return _chunk(c, sizes[c], seed, n_txps, kbar, cdf, g_start, g_size, gene_of, coverage, gaps, fam)

    if n_chunks > 1 and threads > 1:
        with ThreadPoolExecutor(max_workers=threads) as ex:
            parts = list(ex.map(run, range(n_chunks)))
    else:
        parts = [run(c) for c in range(n_chunks)]
    lens = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, dtype=np.uint64)
    row_ptr = np.zeros(n_reads + 1, dtype=np.uint64)
    np.cumsum(lens, out=row_ptr[1:])
    tid = np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, dtype=np.uint32)
    as_prob = np.concatenate([p[2] for p in parts]) if parts else np.zeros(0, dtype=np.float32)
    cov = np.concatenate([p[3] for p in parts]) if coverage and parts else None
    return SyntheticStore(row_ptr, tid, as_prob, cov, n_txps, a, gene_of)


# BASELINE.json configs (C2, C3/C4, C5)
CONFIGS = {
    "c2": dict(n_reads=1_000_000, n_txps=60_000, kbar=8.0),
    "c3": dict(n_reads=10_000_000, n_txps=200_000, kbar=8.0),
    "c5_cell": dict(n_reads=50_000, n_txps=60_000, kbar=8.0),
}


def make_config(name: str, coverage: bool = False, seed_offset: int = 0, **over) -> SyntheticStore:
    cfg = dict(CONFIGS[name])
    cfg.update(over)
    return make_store(seed=BASE_SEED + seed_offset, coverage=coverage, **cfg)


def make_cells(n_cells: int, reads_per_cell: int, n_txps: int, kbar: float = 8.0,
               seed: int = BASE_SEED + 5, expressed_frac: Optional[float] = None, first_cell: int = 0, threads: int = 1):
    """C5: concatenated per-cell stores.  Cell c is a pure function of (seed, c), so ranks that each
    generate a block of cells (``first_cell``) produce pieces of one experiment.

    ``expressed_frac`` (None: every cell draws from all ``n_txps`` transcripts, the benchmark's workload): a cell
    expresses a random subset of that fraction of the annotation -- its store is generated over the subset and mapped
    back through the sorted subset ids, so genes stay runs of neighbouring ids (single-cell data: a cell touches a
    few per cent to a fifth of the transcripts; what the per-cell transcript compaction of the batched store is for)."""
    def one(c):
        cs = seed * 1000 + first_cell + c
        if expressed_frac is None:
            return make_store(reads_per_cell, n_txps, kbar, seed=cs, threads=1)
        n_sub = min(n_txps, max(int(n_txps * expressed_frac), 8))
        sub = np.sort(np.random.default_rng([cs, 0xCE11]).choice(n_txps, n_sub, replace=False)).astype(np.uint32)
        st = make_store(reads_per_cell, n_sub, kbar, seed=cs, threads=1)
        return SyntheticStore(st.row_ptr, sub[st.tid], st.as_prob, None, n_txps, None, None)

    if threads > 1 and n_cells > 1:
        with ThreadPoolExecutor(max_workers=threads) as ex:
            stores = list(ex.map(one, range(n_cells)))
    else:
        stores = [one(c) for c in range(n_cells)]
    rps, tids, ps = [np.zeros(1, dtype=np.uint64)], [], []
    cell_off = np.zeros(n_cells + 1, dtype=np.uint64)
    base = 0
    for c, st in enumerate(stores):
        rps.append(st.row_ptr[1:] + np.uint64(base))
        tids.append(st.tid)
        ps.append(st.as_prob)
        base += st.nnz
        cell_off[c + 1] = cell_off[c] + np.uint64(st.n_reads)
    return (cell_off, np.concatenate(rps), np.concatenate(tids) if tids else np.zeros(0, np.uint32),
            np.concatenate(ps) if ps else np.zeros(0, np.float32))


def make_coordinates(tid, n_txps: int, seed: int = BASE_SEED + 9, zero_span_frac: float = 0.0,
                     min_len: int = 400, max_len: int = 6000, threads: int = 1):
    """Alignment coordinates consistent with a store's transcript ids, so that a store (``make_store``,
    ``make_cells``) can carry a coverage model: (txp_len u64[n_txps], aln_start u32[nnz], aln_end u32[nnz]).

    Transcript lengths are uniform on [min_len, max_len); alignment j of transcript t spans 100 .. 3000 bases
    (at most the transcript) at a uniform position inside it, so 0 <= start <= end <= txp_len[t].  A fraction
    ``zero_span_frac`` of the alignments get end == start (the reference's coverage model gives them NaN).
    Alignments are drawn in chunks of ``CHUNK``, chunk c from ``default_rng([seed, c])``: the result is a pure
    function of (tid, n_txps, seed, zero_span_frac, min_len, max_len)."""
    tid = np.asarray(tid, dtype=np.uint32)
    txp_len = np.random.default_rng([seed, 0x7E4]).integers(min_len, max_len, size=n_txps).astype(np.uint64)
    nnz = len(tid)
    start = np.empty(nnz, dtype=np.uint32)
    end = np.empty(nnz, dtype=np.uint32)

    def one(c):
        a, b = c * CHUNK, min(nnz, (c + 1) * CHUNK)
        rng = np.random.default_rng([seed, c])
        L = txp_len[tid[a:b]].astype(np.int64)
        span = np.minimum(rng.integers(100, 3000, size=b - a), L)
        s = (rng.random(b - a) * (L - span + 1)).astype(np.int64)
        s = np.minimum(s, L - span)
        span = np.where(rng.random(b - a) < zero_span_frac, 0, span)
        start[a:b] = s
        end[a:b] = s + span

    n_chunks = -(-nnz // CHUNK)
    if threads > 1 and n_chunks > 1:
        with ThreadPoolExecutor(max_workers=threads) as ex:
            list(ex.map(one, range(n_chunks)))
    else:
        for c in range(n_chunks):
            one(c)
    return txp_len, start, end


@dataclass
class SyntheticRecords:
    filters: dict                # the fields of oem_filters the records were made for
    txp_len: np.ndarray          # u64 [T]
    records: np.ndarray          # builder.ALN_RECORD [n_records]
    group_off: np.ndarray        # u64 [n_groups + 1]
    kept: np.ndarray             # u32 [n_groups]: what the filter keeps of each group
    discard: dict                # the discard table the filter ends with


def make_records(store: SyntheticStore, seed: int = BASE_SEED + 21, decoy_rate: float = 0.3, drop_frac: float = 0.05,
                 score_prob_denom: float = 5.0, txp_len=None) -> SyntheticRecords:
    """A synthetic store turned back into the alignment records it could have come from, so that
    AlignmentFilters::filter (oarfish_types.rs:955-1130) over the records gives the store again: the same reads in the
    same order, the same transcripts and the same score gaps (``as_prob`` is then libm's expf of the gap, which can
    differ in the last bit from the numpy exp the synthetic store was made with).

    Each kept alignment gets the integer score ``best - g`` that reproduces its ``as_prob = expf(-g / D)`` (g =
    round(-D ln p): the store's probabilities are exp of an integer gap over D, and every read has a g = 0 alignment),
    with the read's best score high enough that ``score / best >= 0.95`` holds with room to spare.  Coordinates are drawn
    inside the transcripts (lengths uniform on [400, 6000)) so that the 5' clip (2000) and the 3' clip (3000) keep them,
    and are usable for the coverage model.  On top of that the generator adds, per read, Poisson(``decoy_rate``) DECOY
    records, each rejected by exactly one filter (orientation, supplementary, aligned length, 3' clip, 5' clip in the
    first walk -- these carry a score above the read's best, which they must not become -- or the score threshold in the
    second), before or after the read's real records; and whole reads that are dropped (``drop_frac`` of the groups:
    unmapped records only, a non-positive best score, or a best alignment that covers too little of the read).
    ``kept`` and ``discard`` are what the filter must report.  A pure function of (store, seed, rates, D).
    ``txp_len`` (lengths of at least 400): the annotation to draw the coordinates in, instead of one drawn here
    (``make_cell_records``: every cell of an experiment has the same)."""
    from .builder import ALN_RECORD, REC_HAS_SCORE, REC_REVERSE, REC_SUPPLEMENTARY, REC_UNMAPPED
    F5, F3 = 2000, 3000
    filters = dict(five_prime_clip=F5, three_prime_clip=F3, score_threshold=0.95, min_aligned_fraction=0.5,
                   min_aligned_len=50, which_strand=1, score_prob_denom=float(score_prob_denom))
    rng = np.random.default_rng([seed, 0xF117E4])
    R, T, nnz = store.n_reads, store.n_txps, store.nnz
    rp = store.row_ptr.astype(np.int64)
    lens = np.diff(rp)
    if R and lens.min() < 1:
        raise ValueError("make_records needs a store without empty reads")
    drawn = rng.integers(400, 6000, size=T).astype(np.uint64)
    txp_len = drawn if txp_len is None else np.ascontiguousarray(txp_len, dtype=np.uint64)
    if len(txp_len) != T or (T and txp_len.min() < 400):
        raise ValueError("make_records needs n_txps transcript lengths of at least 400")
    gap = np.rint(-float(score_prob_denom) * np.log(store.as_prob.astype(np.float64))).astype(np.int64)
    first = rp[:-1]
    if R:
        if np.minimum.reduceat(gap, first).max() != 0:
            raise ValueError("make_records needs a read's best alignment to have as_prob 1")
        gmax = np.maximum.reduceat(gap, first)
    else:
        gmax = np.zeros(0, dtype=np.int64)
    best = 20 * gmax + rng.integers(1000, 3000, size=R)
    read_of = np.repeat(np.arange(R, dtype=np.int64), lens)
    # coordinates of the real alignments: start < min(L - 100, F5), end in (max(start + 100, L - F3), L]
    L = txp_len[store.tid].astype(np.int64)
    start = (rng.random(nnz) * np.minimum(L - 100, F5)).astype(np.int64)
    lo = np.maximum(start + 100, L - F3 + 1)
    end = np.minimum(lo + (rng.random(nnz) * (L - lo + 1)).astype(np.int64), L)
    span = end - start
    # the read's length: the first best alignment covers more than half of it
    is_best = np.flatnonzero(gap == 0)
    _, where = np.unique(read_of[is_best], return_index=True)
    span_best = span[is_best[where]] if R else np.zeros(0, dtype=np.int64)
    seq_len = span_best + (rng.random(R) * span_best).astype(np.int64)
    seq_len = np.minimum(seq_len, 2 * span_best - 1)

    # groups: the R reads in order, with dropped reads scattered between them
    n_drop = int(round(R * drop_frac / max(1e-9, 1.0 - drop_frac))) if R else 0
    G = R + n_drop
    is_real = np.ones(G, dtype=bool)
    if n_drop:
        is_real[rng.choice(G, size=n_drop, replace=False)] = False
    drop_kind = rng.integers(0, 3, size=n_drop)
    nd = rng.poisson(decoy_rate, size=R).astype(np.int64)
    nf = rng.binomial(nd, 0.5).astype(np.int64)                        # decoys in front of the real records
    n_rec = np.zeros(G, dtype=np.int64)
    n_rec[is_real] = lens + nd
    n_rec[~is_real] = np.where(drop_kind == 0, 2, 1)
    group_off = np.zeros(G + 1, dtype=np.uint64)
    np.cumsum(n_rec, out=group_off[1:])
    base_real = group_off[:-1][is_real].astype(np.int64)
    base_drop = group_off[:-1][~is_real].astype(np.int64)
    rec = np.zeros(int(group_off[-1]), dtype=ALN_RECORD)
    rec["seq_len"] = -1

    # the real records
    pos = np.repeat(base_real + nf, lens) + (np.arange(nnz, dtype=np.int64) - np.repeat(first, lens))
    rec["ref_id"][pos] = store.tid
    rec["aln_start"][pos] = start
    rec["aln_end"][pos] = end
    rec["aln_span"][pos] = span
    rec["score"][pos] = best[read_of] - gap
    rec["seq_len"][pos] = seq_len[read_of]
    rec["flags"][pos] = REC_HAS_SCORE

    # the decoys: kind 0 orientation, 1 supplementary, 2 aligned length, 3 3' clip, 4 5' clip, 5 score threshold
    n_dec = int(nd.sum())
    d_read = np.repeat(np.arange(R, dtype=np.int64), nd)
    q = np.arange(n_dec, dtype=np.int64) - np.repeat(np.cumsum(nd) - nd, nd)
    d_pos = base_real[d_read] + np.where(q < nf[d_read], q, lens[d_read] + q)
    d_tid = rng.integers(0, T, size=n_dec)
    d_L = txp_len[d_tid].astype(np.int64)
    kind = rng.integers(0, 6, size=n_dec)
    kind = np.where((kind == 3) & (d_L < F3), 1, kind)                 # (no 3' decoy on a transcript shorter than the clip)
    rec["ref_id"][d_pos] = d_tid
    rec["aln_start"][d_pos] = np.where(kind == 4, F5, 0)
    rec["aln_end"][d_pos] = np.where(kind == 3, d_L - F3, d_L)
    rec["aln_span"][d_pos] = np.where(kind == 2, 10, 100)
    rec["score"][d_pos] = np.where(kind == 5, best[d_read] * 9 // 10, best[d_read] + 50)
    rec["seq_len"][d_pos] = seq_len[d_read]
    rec["flags"][d_pos] = REC_HAS_SCORE | np.where(kind == 0, REC_REVERSE, 0) | np.where(kind == 1, REC_SUPPLEMENTARY, 0)

    # the dropped reads: 0 = two unmapped records (their ref_id is never looked at), 1 = best score 0, 2 = the best
    # alignment covers a tenth of the read
    for k in range(3):
        b = base_drop[drop_kind == k]
        if k == 0:
            for j in (0, 1):
                rec["ref_id"][b + j] = 0xFFFFFFFF
                rec["flags"][b + j] = REC_UNMAPPED
        else:
            t = rng.integers(0, T, size=len(b))
            rec["ref_id"][b] = t
            rec["aln_end"][b] = txp_len[t]
            rec["aln_span"][b] = 100
            rec["score"][b] = 0 if k == 1 else 1000
            rec["seq_len"][b] = 100 if k == 1 else 1000
            rec["flags"][b] = REC_HAS_SCORE
    kept = np.zeros(G, dtype=np.uint32)
    kept[is_real] = lens
    discard = dict(discard_5p=int((kind == 4).sum()), discard_3p=int((kind == 3).sum()), discard_score=int((kind == 5).sum()),
                   discard_aln_frac=int((drop_kind == 2).sum()), discard_aln_len=int((kind == 2).sum()),
                   discard_ori=int((kind == 0).sum()), discard_supp=int((kind == 1).sum()), valid_best_aln=R,
                   no_mapping=int((drop_kind == 0).sum()), no_valid_aln=int((drop_kind == 1).sum()))
    return SyntheticRecords(filters, txp_len, rec, group_off, kept, discard)


@dataclass
class SyntheticCellRecords:
    filters: dict                # the fields of oem_filters the records were made for
    txp_len: np.ndarray          # u64 [T]: one annotation for all cells
    records: np.ndarray          # builder.ALN_RECORD [n_records]: the cells' records one after the other
    group_off: np.ndarray        # u64 [n_groups + 1]
    cell_group_off: np.ndarray   # u64 [n_cells + 1]: cell c owns the groups cell_group_off[c] : cell_group_off[c + 1]
    kept: np.ndarray             # u32 [n_groups]
    discard: list                # one discard table (dict) per cell


def make_cell_records(cells, n_txps: int, seed: int = BASE_SEED + 23, threads: int = 1, **kw) -> SyntheticCellRecords:
    """``make_records`` per cell of ``cells = make_cells(...)`` (``(cell_row_off, row_ptr, tid, as_prob)``), concatenated:
    the input of ``em_cells_records_sparse``.  Cell c's records are a pure function of (the cell's store, seed, c, the
    keyword arguments of ``make_records``); all cells share one annotation, drawn from ``seed``.  A cell without reads
    has no groups."""
    from .builder import ALN_RECORD
    cell_off, row_ptr, tid, p = cells
    n_cells = len(cell_off) - 1
    txp_len = np.random.default_rng([seed, 0x7E4]).integers(400, 6000, size=n_txps).astype(np.uint64)
    recs, goffs, kepts, tables = [], [np.zeros(1, dtype=np.uint64)], [], []
    cgo = np.zeros(n_cells + 1, dtype=np.uint64)
    filters, base = None, 0

    def one(c):
        r0, r1 = int(cell_off[c]), int(cell_off[c + 1])
        a0, a1 = int(row_ptr[r0]), int(row_ptr[r1])
        st = SyntheticStore(row_ptr[r0:r1 + 1] - row_ptr[r0], tid[a0:a1], p[a0:a1], None, n_txps, None, None)
        return make_records(st, seed=seed * 1000 + c, txp_len=txp_len, **kw)

    if threads > 1 and n_cells > 1:
        with ThreadPoolExecutor(max_workers=threads) as ex:
            per_cell = list(ex.map(one, range(n_cells)))
    else:
        per_cell = (one(c) for c in range(n_cells))
    for c, sr in enumerate(per_cell):
        filters = sr.filters
        recs.append(sr.records)
        goffs.append(sr.group_off[1:] + np.uint64(base))
        kepts.append(sr.kept)
        tables.append(sr.discard)
        base += len(sr.records)
        cgo[c + 1] = cgo[c] + np.uint64(len(sr.group_off) - 1)
    if filters is None:
        filters = make_records(SyntheticStore(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32), None,
                                              n_txps, None, None), seed=seed, txp_len=txp_len, **kw).filters
    return SyntheticCellRecords(filters, txp_len, np.concatenate(recs) if recs else np.zeros(0, dtype=ALN_RECORD),
                                np.concatenate(goffs), cgo, np.concatenate(kepts) if kepts else np.zeros(0, np.uint32), tables)


_HEX = np.frombuffer(b"0123456789abcdef", dtype=np.uint8)
_ILLUMINA_PREFIX = b"A00741:132:HJ3KVDSX2:"
_ILLUMINA_XY = 31000   # x and y run over [1000, 32000): four or five digits


def _coprime_multiplier(rng: np.random.Generator, m: int) -> int:
    import math
    while True:
        a = int(rng.integers(1 << 16, 1 << 20)) | 1
        if math.gcd(a, m) == 1:
            return a


def make_record_names(group_off, style: str = "uuid", seed: int = BASE_SEED + 24):
    """Read names for grouped records: one name per group, distinct between groups, repeated for every record of the
    group.  Returns ``(blob uint8, offsets uint64[n_records + 1])``, what ``types.pack_read_names`` passes through.

    ``style="uuid"``: 36 bytes, lower-case hex with dashes, as ONT reads carry them -- random from the first byte on.
    ``style="illumina"``: ``instrument:run:flowcell:lane:tile:x:y`` with one instrument, run and flowcell, so that all
    names share their first 21 bytes and differ in length (37 to 39 bytes)."""
    group_off = np.ascontiguousarray(group_off, dtype=np.uint64)
    per_group = _group_names(len(group_off) - 1, style, seed)
    return _flatten_names(np.repeat(per_group, np.diff(group_off).astype(np.int64), axis=0))


def _flatten_names(per_record):
    """Rows of name bytes, 0 where a name has no byte -> (blob, offsets)."""
    present = per_record != 0
    off = np.zeros(len(per_record) + 1, dtype=np.uint64)
    np.cumsum(present.sum(axis=1, dtype=np.uint64), out=off[1:])
    return per_record[present], off


def _group_names(n_groups: int, style: str, seed: int):
    """One row of name bytes per group (0: no byte there)."""
    rng = np.random.default_rng([seed, 0xC011])
    if style == "uuid":
        raw = rng.integers(0, 256, size=(n_groups, 16), dtype=np.uint8)
        with np.errstate(over="ignore"):   # times an odd number modulo 2^64: a bijection, so the names are distinct
            head = (np.arange(n_groups, dtype=np.uint64) * np.uint64(int(rng.integers(1 << 62, 1 << 63)) | 1)
                    + np.uint64(rng.integers(0, 1 << 63)))
        raw[:, :8] = head.view(np.uint8).reshape(n_groups, 8)
        hx = np.empty((n_groups, 32), dtype=np.uint8)
        hx[:, 0::2] = _HEX[raw >> 4]
        hx[:, 1::2] = _HEX[raw & 15]
        per_group = np.full((n_groups, 36), ord("-"), dtype=np.uint8)
        for dst, src, w in ((0, 0, 8), (9, 8, 4), (14, 12, 4), (19, 16, 4), (24, 20, 12)):
            per_group[:, dst:dst + w] = hx[:, src:src + w]
    elif style == "illumina":
        modulus = 4 * 64 * _ILLUMINA_XY * _ILLUMINA_XY
        if n_groups > modulus:
            raise ValueError("too many groups for distinct illumina-style names")
        u = (np.arange(n_groups, dtype=np.uint64) * np.uint64(_coprime_multiplier(rng, modulus))
             + np.uint64(rng.integers(0, modulus))) % np.uint64(modulus)   # a bijection of [0, modulus): names stay distinct
        x = u % np.uint64(_ILLUMINA_XY) + np.uint64(1000)
        u //= np.uint64(_ILLUMINA_XY)
        y = u % np.uint64(_ILLUMINA_XY) + np.uint64(1000)
        u //= np.uint64(_ILLUMINA_XY)
        tile = u % np.uint64(64) + np.uint64(1101)
        lane = u // np.uint64(64) + np.uint64(1)
        pre = np.frombuffer(_ILLUMINA_PREFIX, dtype=np.uint8)
        per_group = np.zeros((n_groups, len(pre) + 1 + 1 + 4 + 1 + 5 + 1 + 5), dtype=np.uint8)   # 0: no byte here
        per_group[:, :len(pre)] = pre
        col = len(pre)

        def digits(v, width, at):
            for k in range(width):
                d = (v // np.uint64(10 ** (width - 1 - k))) % np.uint64(10)
                lead = v < np.uint64(10 ** (width - 1 - k))
                per_group[:, at + k] = np.where(lead & (k < width - 1), 0, d.astype(np.uint8) + ord("0"))
            return at + width

        col = digits(lane, 1, col)
        per_group[:, col] = ord(":")
        col = digits(tile, 4, col + 1)
        per_group[:, col] = ord(":")
        col = digits(x, 5, col + 1)
        per_group[:, col] = ord(":")
        digits(y, 5, col + 1)
    else:
        raise ValueError(f"style must be 'uuid' or 'illumina', not {style!r}")
    return per_group


def make_named_records(synthetic_records: SyntheticRecords, style: str = "uuid", seed: int = BASE_SEED + 28,
                       unmapped_rate: float = 0.0, shuffle: bool = False):
    """``make_records``' groups as a BAM reader hands them to the bulk parser (alignment_parser.rs:301-437): every record
    with its read's name (``make_record_names``), the first record of a group the read's primary alignment and the
    others carrying the secondary flag.  ``unmapped_rate``: that many extra UNMAPPED records per record, sprinkled inside
    and between the reads, half of them with a name of their own and half with an empty name -- the parser skips them
    before it groups, so they cut no read.  ``shuffle``: the whole input permuted (what ``mode="sort"`` is for).
    Returns ``(records, names, secondary)`` in input order, ``names`` a ``(blob, offsets)`` pair: the input of
    ``DeviceStore.from_named_records``.  A pure function of its arguments."""
    from .builder import REC_UNMAPPED
    sr = synthetic_records
    group_off = np.ascontiguousarray(sr.group_off, dtype=np.uint64)
    sizes = np.diff(group_off).astype(np.int64)
    n = int(group_off[-1])
    rows = np.repeat(_group_names(len(sizes), style, seed), sizes, axis=0)
    records = sr.records[:n]
    secondary = np.ones(n, dtype=np.uint8)
    secondary[group_off[:-1][sizes > 0].astype(np.int64)] = 0
    rng = np.random.default_rng([seed, 0x0A3ED])
    k = int(round(float(unmapped_rate) * n))
    if k:
        at = np.sort(rng.integers(0, n + 1, size=k))          # an extra record goes in front of record at[j]
        extra = np.zeros(k, dtype=records.dtype)
        extra["ref_id"] = 0xFFFFFFFF
        extra["flags"] = REC_UNMAPPED
        extra_rows = _group_names(k, style, seed + 1)
        extra_rows[rng.random(k) < 0.5] = 0                     # half of them have no name at all
        records = np.insert(records, at, extra)
        rows = np.insert(rows, at, extra_rows, axis=0)
        secondary = np.insert(secondary, at, np.zeros(k, dtype=np.uint8))
    if shuffle:
        perm = rng.permutation(len(records))
        records, rows, secondary = records[perm], rows[perm], secondary[perm]
    return np.ascontiguousarray(records), _flatten_names(rows), np.ascontiguousarray(secondary)


def cut_named_records(records, names, cuts, secondary=None):
    """``make_named_records``' input cut into batches for a names session (``RecordsStream(names=True)``): ``cuts`` are
    record positions, in any order and with repeats (a repeat gives an empty batch); 0 and ``len(records)`` are implied.
    A cut may fall inside a read.  Returns a list of ``(records, (blob, offsets))``, the offsets of each batch from 0;
    with ``secondary`` (one flag per record, for a sorting names session) a list of ``(records, (blob, offsets),
    secondary)``.  A pure function of its arguments."""
    records = np.asarray(records)
    blob, off = np.asarray(names[0], dtype=np.uint8), np.asarray(names[1], dtype=np.uint64)
    n = len(records)
    if len(off) != n + 1:
        raise ValueError("names must have one entry per record")
    edges = [0] + sorted(int(c) for c in cuts) + [n]
    if edges[1] < 0 or edges[-2] > n:
        raise ValueError("a cut lies outside the records")
    if secondary is not None:
        secondary = np.asarray(secondary)
        if len(secondary) != n:
            raise ValueError("secondary must have one entry per record")
    out = []
    for a, b in zip(edges[:-1], edges[1:]):
        o = off[a:b + 1]
        batch = (np.ascontiguousarray(records[a:b]),
                 (np.ascontiguousarray(blob[int(o[0]):int(o[-1])]), np.ascontiguousarray(o - o[0])))
        out.append(batch if secondary is None else batch + (np.ascontiguousarray(secondary[a:b]),))
    return out


def shuffle_cell_records(cell_records: SyntheticCellRecords, seed: int = BASE_SEED + 25, style: str = "uuid", threads: int = 1,
                         with_records: bool = True):
    """``make_cell_records``' cells as a barcode-collated input holds them: every cell's records permuted, each with its
    read's name (``make_record_names``; distinct between the reads of a cell).  The first record of a group is the
    read's primary alignment, the others carry the secondary flag.  Returns ``(records, names, secondary,
    cell_rec_off)`` -- ``names`` a ``(blob, offsets)`` pair --, the input of ``em.collate_names`` and of
    ``em_cells_records_sparse(..., names=, secondary=)``.  Cell c's share is a pure function of (its groups, seed, c,
    style).  ``with_records=False`` leaves the records alone and returns None in their place."""
    cr = cell_records
    group_off = np.ascontiguousarray(cr.group_off, dtype=np.uint64)
    cgo = np.ascontiguousarray(cr.cell_group_off, dtype=np.int64)
    n_cells = len(cgo) - 1
    cell_rec_off = group_off[cgo]

    def one(c):
        goff = group_off[cgo[c]:cgo[c + 1] + 1] - group_off[cgo[c]]
        n = int(goff[-1])
        group_of = np.repeat(np.arange(len(goff) - 1), np.diff(goff).astype(np.int64))
        secondary = np.ones(n, dtype=np.uint8)
        secondary[goff[:-1][np.diff(goff) > 0].astype(np.int64)] = 0
        perm = np.random.default_rng([seed, 0x5AFF, c]).permutation(n)
        blob, off = _flatten_names(_group_names(len(goff) - 1, style, seed * 1000 + c)[group_of[perm]])
        return perm + int(cell_rec_off[c]), blob, np.diff(off), secondary[perm]

    if threads > 1 and n_cells > 1:
        with ThreadPoolExecutor(max_workers=threads) as ex:
            per_cell = list(ex.map(one, range(n_cells)))
    else:
        per_cell = [one(c) for c in range(n_cells)]
    n = int(cell_rec_off[-1])
    off = np.zeros(n + 1, dtype=np.uint64)
    if per_cell:
        np.cumsum(np.concatenate([x[2] for x in per_cell]), out=off[1:])
    blob = np.concatenate([x[1] for x in per_cell]) if per_cell else np.zeros(0, dtype=np.uint8)
    secondary = np.concatenate([x[3] for x in per_cell]) if per_cell else np.zeros(0, dtype=np.uint8)
    records = None
    if with_records:
        records = cr.records[np.concatenate([x[0] for x in per_cell])] if per_cell else cr.records[:0]
    return records, (blob, off), secondary, cell_rec_off


_NUC = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_barcodes(n_cells: int, style: str = "10x", seed: int = BASE_SEED + 26) -> list:
    """``n_cells`` distinct cell barcodes, as ``bytes``.

    ``style="10x"``: 16 nucleotides and ``-1``, 18 bytes: three 8-byte key rounds of the device sort.
    ``style="var"``: lengths 1 to 20 over ``ACGT``; every third barcode is a proper prefix of its predecessor where
    that still gives a new one, so prefixes of other barcodes occur."""
    rng = np.random.default_rng([seed, 0xBA2C])
    out, seen = [], set()
    if style == "10x":
        while len(out) < n_cells:
            b = _NUC[rng.integers(0, 4, size=16)].tobytes() + b"-1"
            if b not in seen:
                seen.add(b)
                out.append(b)
    elif style == "var":
        while len(out) < n_cells:
            b = _NUC[rng.integers(0, 4, size=int(rng.integers(1, 21)))].tobytes()
            if len(out) % 3 == 2 and len(out[-1]) > 1:
                pre = out[-1][:int(rng.integers(1, len(out[-1])))]
                b = pre if pre not in seen else b
            if b not in seen:
                seen.add(b)
                out.append(b)
    else:
        raise ValueError(f"style must be '10x' or 'var', not {style!r}")
    return out


def interleave_cells(records, names, secondary, cell_rec_off, barcodes, seed: int = BASE_SEED + 27, how: str = "uniform"):
    """``shuffle_cell_records``' barcode-collated input as an UNCOLLATED input: the records of all cells interleaved,
    each with its cell's barcode.  ``barcodes``: one per cell (``make_barcodes``).  ``how="uniform"``: a uniform
    permutation of all records.  ``how="blocks"``: every cell's records are cut into runs of 1 to 8 and the runs of all
    cells shuffled: a few records of a cell side by side, as a coordinate-sorted file interleaves cells.  Returns ``(records, names,
    secondary, record_barcodes, perm)``: ``names`` and ``record_barcodes`` are ``(blob, offsets)`` pairs and ``perm[k]``
    is the collated index of the record at input position k.  ``records`` / ``secondary`` may be None."""
    from .em import gather_names
    cell_rec_off = np.ascontiguousarray(cell_rec_off, dtype=np.int64)
    n, n_cells = int(cell_rec_off[-1]), len(cell_rec_off) - 1
    if len(barcodes) != n_cells:
        raise ValueError("one barcode per cell")
    rng = np.random.default_rng([seed, 0x1EAF])
    if how == "uniform":
        perm = rng.permutation(n)
    elif how == "blocks":
        starts = []
        for c in range(n_cells):
            at, end = int(cell_rec_off[c]), int(cell_rec_off[c + 1])
            while at < end:
                w = min(int(rng.integers(1, 9)), end - at)
                starts.append((at, w))
                at += w
        pick = rng.permutation(len(starts))
        perm = (np.concatenate([np.arange(starts[i][0], starts[i][0] + starts[i][1]) for i in pick]) if starts
                else np.zeros(0, dtype=np.int64))
    else:
        raise ValueError(f"how must be 'uniform' or 'blocks', not {how!r}")
    perm = perm.astype(np.int64)
    cell_of = np.repeat(np.arange(n_cells), np.diff(cell_rec_off))[perm]
    enc = [b.encode() if isinstance(b, str) else bytes(b) for b in barcodes]
    bc_off = np.zeros(n_cells + 1, dtype=np.int64)
    np.cumsum([len(b) for b in enc], out=bc_off[1:])
    bc_blob = np.frombuffer(b"".join(enc), dtype=np.uint8)
    return (None if records is None else records[perm], gather_names(names, perm),
            None if secondary is None else np.asarray(secondary)[perm], gather_names((bc_blob, bc_off), cell_of), perm)


def gene_of_txps(n_txps: int, seed: int = BASE_SEED + 31):
    """A synthetic annotation for the UMI rule: one ``uint32`` gene id per transcript, genes of 1 + Geom(1/4) consecutive
    transcripts (``_genes``, the gene model of the synthetic stores).  A pure function of its arguments."""
    return _genes(int(n_txps), np.random.default_rng([seed, 0x6E4E]))[2].astype(np.uint32)


def _mix64(x):
    """splitmix64's finalizer over a ``uint64`` array."""
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _string_hashes(pair, n):
    """A 64-bit hash of every string of a ``(blob, offsets)`` pair (polynomial in the bytes, then mixed)."""
    blob, off = np.asarray(pair[0], dtype=np.uint8), np.ascontiguousarray(pair[1], dtype=np.int64)
    if len(off) != n + 1:
        raise ValueError("one entry per record is needed")
    lens = np.diff(off)
    h = np.zeros(n, dtype=np.uint64)
    total = int(off[-1] - off[0])
    if total:
        pos = np.arange(total, dtype=np.int64) - np.repeat(off[:-1] - off[0], lens)
        table = np.ones(int(lens.max()) + 1, dtype=np.uint64)
        np.multiply.accumulate(np.full(len(table) - 1, 0x100000001B3, dtype=np.uint64), out=table[1:])
        terms = (blob[int(off[0]):int(off[-1])].astype(np.uint64) + np.uint64(1)) * table[pos]
        full = lens > 0
        h[full] = np.add.reduceat(terms, (off[:-1] - off[0])[full])
    return _mix64(h ^ lens.astype(np.uint64))


def add_umi_errors(umis, rate: float, seed: int = BASE_SEED + 37, names=None, barcodes=None):
    """Sequencing errors in the UMIs of an input (``add_umi_duplicates``' ``umis``): in a fraction ``rate`` of the READS one
    nucleotide of the UMI is substituted by another of ``ACGT``, the same substitution on all records of the read.  A read
    is the records that share a barcode and a name (``names`` / ``barcodes``: ``(blob, offsets)`` pairs, one entry per
    record); without them every record is a read of its own.  A PCR copy has its own name, so a copy may carry an error
    its original does not: what one-mismatch correction (``dedup_umis_rule(correct=True)``) undoes.  Which reads are hit,
    where and by what depends on the seed, the read's barcode and name and -- without names -- the record's index only,
    not on the order of the records.  Empty UMIs stay empty.  Returns the new ``(blob, offsets)`` pair."""
    if not 0.0 <= rate <= 1.0:
        raise ValueError("rate must be in [0, 1]")
    blob, off = np.array(umis[0], dtype=np.uint8), np.ascontiguousarray(umis[1], dtype=np.int64)
    n = len(off) - 1
    key = np.arange(n, dtype=np.uint64) if names is None else _string_hashes(names, n)
    if barcodes is not None:
        key = _mix64(key ^ (_string_hashes(barcodes, n) * np.uint64(0x9E3779B97F4A7C15)))
    h = _mix64(key ^ _mix64(np.full(n, int(seed) & (2 ** 64 - 1), dtype=np.uint64)))
    lens = np.diff(off)
    hit = ((h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 < rate) & (lens > 0)
    idx = np.flatnonzero(hit)
    h2 = _mix64(h[idx] + np.uint64(1))
    at = off[idx] - off[0] + (h2 % lens[idx].astype(np.uint64)).astype(np.int64)
    old = blob[at]
    was = np.argmax(old[:, None] == _NUC[None, :], axis=1)               # (a byte outside ACGT counts as A's place)
    new = _NUC[(was + 1 + ((h2 >> np.uint64(32)) % np.uint64(3)).astype(np.int64)) % 4]
    new = np.where(new == old, _NUC[(was + 1) % 4], new)
    blob[at] = new
    return blob, np.ascontiguousarray(umis[1], dtype=np.uint64)


def make_whitelist(n: int, length: int = 16, seed: int = BASE_SEED + 41):
    """A barcode whitelist (a chemistry's permit list) for ``correct_barcodes``: ``n`` distinct labels of ``length``
    nucleotides as a ``(blob, offsets)`` pair.  About an eighth of the labels are made from others by one substitution and
    as many by two, so the list holds pairs at distance 1 (a raw barcode between them is ambiguous, and an error can turn
    one label into another) and at distance 2 (one barcode is a neighbour of both).  A pure function of its arguments."""
    if n < 1 or length < 1 or length > 64 or (length < 32 and n > 4 ** length):
        raise ValueError("make_whitelist needs 1 <= length <= 64 and room for n distinct labels")
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 4, size=(n, length), dtype=np.uint8)
    k = n // 8
    for dist, at in ((1, n - 2 * k), (2, n - k)):
        if k and length >= dist:
            rows[at:at + k] = rows[:k]
            cols = np.argsort(rng.random((k, length)), axis=1)[:, :dist]
            for d in range(dist):
                rows[at + np.arange(k), cols[:, d]] = (rows[np.arange(k), cols[:, d]] + rng.integers(1, 4, size=k, dtype=np.uint8)) % 4
    while True:   # repeated labels are drawn again until none is left
        if length <= 32:   # two bits a nucleotide: a label is one word
            codes = (rows.astype(np.uint64) << (np.uint64(2) * np.arange(length, dtype=np.uint64))[None, :]).sum(axis=1, dtype=np.uint64)
            _, first = np.unique(codes, return_index=True)
        else:
            _, first = np.unique(rows, axis=0, return_index=True)
        again = np.setdiff1d(np.arange(n), first)
        if not len(again):
            break
        rows[again] = rng.integers(0, 4, size=(len(again), length), dtype=np.uint8)
    rows = rows[rng.permutation(n)]
    return np.ascontiguousarray(_NUC[rows].reshape(-1)), np.arange(n + 1, dtype=np.uint64) * np.uint64(length)


def add_barcode_errors(barcodes, rate: float, n_rate: float = 0.0, seed: int = BASE_SEED + 43, names=None):
    """Sequencing errors in the cell barcodes of an input, what ``correct_barcodes`` undoes: in a fraction ``rate`` of the
    READS one nucleotide of the barcode is substituted by another of ``ACGT``, in a further fraction ``n_rate`` one is
    replaced by ``N``; the same on all records of the read.  A read is the records that share a barcode and a name
    (``names``: a ``(blob, offsets)`` pair, one entry per record); without names every record is a read of its own.  Which
    reads are hit, where and by what depends on the seed, the read's barcode and name and -- without names -- the record's
    index only, not on the order of the records.  Empty barcodes stay empty.  Returns the new ``(blob, offsets)`` pair."""
    if not (0.0 <= rate <= 1.0 and 0.0 <= n_rate <= 1.0 and rate + n_rate <= 1.0):
        raise ValueError("rate, n_rate and their sum must be in [0, 1]")
    blob, off = np.array(barcodes[0], dtype=np.uint8), np.ascontiguousarray(barcodes[1], dtype=np.int64)
    n = len(off) - 1
    key = _string_hashes(barcodes, n) * np.uint64(0x9E3779B97F4A7C15)
    key = _mix64(key ^ (np.arange(n, dtype=np.uint64) if names is None else _string_hashes(names, n)))
    h = _mix64(key ^ _mix64(np.full(n, int(seed) & (2 ** 64 - 1), dtype=np.uint64)))
    lens = np.diff(off)
    u = (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    idx = np.flatnonzero((u < rate + n_rate) & (lens > 0))
    h2 = _mix64(h[idx] + np.uint64(1))
    at = off[idx] - off[0] + (h2 % lens[idx].astype(np.uint64)).astype(np.int64)
    old = blob[at]
    was = np.argmax(old[:, None] == _NUC[None, :], axis=1)               # (a byte outside ACGT counts as A's place)
    new = _NUC[(was + 1 + ((h2 >> np.uint64(32)) % np.uint64(3)).astype(np.int64)) % 4]
    new = np.where(new == old, _NUC[(was + 1) % 4], new)
    blob[at] = np.where(u[idx] < rate, new, np.uint8(ord("N")))
    return blob, np.ascontiguousarray(barcodes[1], dtype=np.uint64)


def add_umi_duplicates(records, names, secondary, barcodes, rate: float, seed: int = BASE_SEED + 29, umi_len: int = 12):
    """An uncollated single-cell input (``interleave_cells``) given UMIs and PCR duplicates, the input of
    ``em_cells_records_sparse(..., barcodes=, names=, umis=)``.  ``names`` and ``barcodes`` are ``(blob, offsets)`` pairs,
    one entry per record; a read is the records of one barcode that share a name.

    Every read gets a UMI of ``umi_len`` nucleotides, the same on all its records, that is unique inside its cell by
    construction: the read's rank in its cell through an odd multiplier modulo ``4 ** umi_len``, written in base 4.  A
    fraction ``rate`` of the reads that have no unmapped record is copied 1 to 3 times: identical records and flags, the
    same barcode and UMI, a fresh name (the read's, ``~`` and the copy's number).  The copied records are inserted at
    random record positions; the original records keep their relative order.

    Returns ``(records, names, secondary, barcodes, umis, copies)``: the augmented arrays, ``umis`` a ``(blob, offsets)``
    pair, and ``copies`` a dict from barcode (``bytes``) to the number of copied READS it received -- what deduplication
    has to drop from that cell.  A pure function of its arguments."""
    from .em import gather_names
    if not 0.0 <= rate <= 1.0:
        raise ValueError("rate must be in [0, 1]")
    if not 1 <= umi_len <= 31:
        raise ValueError("umi_len must be in [1, 31]")
    blob, off = np.asarray(names[0], dtype=np.uint8), np.ascontiguousarray(names[1], dtype=np.int64)
    bc_blob, bc_off = np.asarray(barcodes[0], dtype=np.uint8), np.ascontiguousarray(barcodes[1], dtype=np.int64)
    n = len(records)
    if len(off) != n + 1 or len(bc_off) != n + 1:
        raise ValueError("names and barcodes must have one entry per record")

    def padded(b, o, lead=0):
        """The strings as the rows of a zero-padded matrix (none holds a 0 byte), behind `lead` free columns."""
        lens = np.diff(o)
        mat = np.zeros((n, lead + int(lens.max(initial=0))), dtype=np.uint8)
        rows = np.repeat(np.arange(n), lens)
        mat[rows, lead + np.arange(int(o[-1]) - int(o[0])) - np.repeat(o[:-1] - o[0], lens)] = b[int(o[0]):int(o[-1])]
        return mat

    def distinct(mat):
        """(the distinct rows, every row's index among them).  The rows are told apart by a 64-bit hash -- sorting words is
        far cheaper than sorting rows -- and then compared with their group's first row, so a collision is an error, not
        a wrong answer.  The distinct rows come in the order of their hashes: fixed by the rows, not by their order."""
        if not mat.shape[1]:
            return mat[:min(n, 1)], np.zeros(n, dtype=np.int64)
        w = -(-mat.shape[1] // 8)
        words = np.zeros((n, 8 * w), dtype=np.uint8)
        words[:, :mat.shape[1]] = mat
        words = words.view(np.uint64)
        mults = np.random.default_rng(0x5EED).integers(1, 2 ** 63, size=w, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        h = np.zeros(n, dtype=np.uint64)
        for k in range(w):
            h = (h ^ words[:, k]) * mults[k]
            h ^= h >> np.uint64(29)
        _, first, inv = np.unique(h, return_index=True, return_inverse=True)
        inv = inv.reshape(-1).astype(np.int64)
        if not np.array_equal(words[first[inv]], words):
            raise RuntimeError("two different strings share a hash: change the hash's seed")
        return mat[first], inv

    # the cells, then the reads: a read's key is its cell's number (4 bytes, big-endian) and its name
    cell_rows, cell_of = distinct(padded(bc_blob, bc_off))
    cell_label = [r.tobytes().rstrip(b"\0") for r in cell_rows]
    key = padded(blob, off, lead=4)
    key[:, :4] = cell_of.astype(">u4").view(np.uint8).reshape(n, 4)
    read_rows, read_of = distinct(key)
    n_reads = len(read_rows) if n else 0
    read_cell = (np.ascontiguousarray(read_rows[:, :4]).view(">u4").reshape(-1).astype(np.int64) if n_reads
                 else np.zeros(0, dtype=np.int64))
    cell_reads = np.bincount(read_cell, minlength=len(cell_label))
    first_read = np.zeros(len(cell_label) + 1, dtype=np.int64)
    np.cumsum(cell_reads, out=first_read[1:])
    by_cell = np.argsort(read_cell, kind="stable")
    read_rank = np.empty(n_reads, dtype=np.int64)                              # a read's rank among the reads of its cell
    read_rank[by_cell] = np.arange(n_reads, dtype=np.int64) - first_read[read_cell[by_cell]]
    if cell_reads.max(initial=0) > 4 ** umi_len:
        raise ValueError("umi_len is too short for the largest cell")
    rng = np.random.default_rng([seed, 0xD0B1])
    mult, add = 2 * int(rng.integers(0, 4 ** umi_len // 2)) + 1, int(rng.integers(0, 4 ** umi_len))
    mask = np.uint64(4 ** umi_len - 1)
    vals = (read_rank.astype(np.uint64) * np.uint64(mult) + np.uint64(add)) & mask     # (wraps mod 2^64: a multiple of 4^umi_len)
    umi_of_read = _NUC[((vals[:, None] >> (2 * np.arange(umi_len, dtype=np.uint64))[None, :]) & np.uint64(3)).astype(np.int64)]

    unmapped = np.bincount(read_of, weights=(np.asarray(records["flags"]) & 1) != 0, minlength=n_reads) > 0   # OEM_REC_UNMAPPED
    n_copies = np.where((rng.random(n_reads) < rate) & ~unmapped, rng.integers(1, 4, size=n_reads), 0)
    per_cell = np.bincount(read_cell, weights=n_copies, minlength=len(cell_label)).astype(np.int64)
    copies = {cell_label[c]: int(k) for c, k in enumerate(per_cell) if k}
    # a copied read's records, each as often as its read is copied; the copy's number is its place among those repeats
    by_read = np.argsort(read_of, kind="stable")
    reps = n_copies[read_of[by_read]]
    src = np.repeat(by_read, reps)
    starts = np.zeros(len(by_read) + 1, dtype=np.int64)
    np.cumsum(reps, out=starts[1:])
    copy_no = np.arange(len(src), dtype=np.int64) - np.repeat(starts[:-1], reps) + 1
    # their names: the read's, "~" and the number
    cblob, coff = gather_names((blob, off), src)
    coff = coff.astype(np.int64)
    new_off = coff + 2 * np.arange(len(src) + 1, dtype=np.int64)
    new_blob = np.empty(int(new_off[-1]), dtype=np.uint8)
    new_blob[np.arange(int(coff[-1]), dtype=np.int64) + 2 * np.repeat(np.arange(len(src), dtype=np.int64), np.diff(coff))] = cblob
    new_blob[new_off[1:] - 2] = ord("~")
    new_blob[new_off[1:] - 1] = 48 + copy_no
    where = np.concatenate([np.arange(n, dtype=np.float64), rng.uniform(0.0, float(max(n, 1)), size=len(src))])
    perm = np.argsort(where, kind="stable")
    src_all = np.concatenate([np.arange(n, dtype=np.int64), src])[perm]
    all_names = (np.concatenate([blob[int(off[0]):int(off[-1])], new_blob]), np.concatenate([off - off[0], int(off[-1] - off[0]) + new_off[1:]]))
    umis = (np.ascontiguousarray(umi_of_read[read_of[src_all]]).reshape(-1),
            np.arange(len(src_all) + 1, dtype=np.uint64) * np.uint64(umi_len))
    return (np.ascontiguousarray(records[src_all]), gather_names(all_names, perm),
            None if secondary is None else np.ascontiguousarray(np.asarray(secondary)[src_all]),
            gather_names((bc_blob, bc_off), src_all), umis, copies)


def recollate_by_first_barcode(record_barcodes):
    """The stable permutation that makes an uncollated stream barcode-collated: the records ordered by the first
    occurrence of their barcode, the records of one barcode keeping their order.  ``record_barcodes`` is a ``(blob,
    offsets)`` pair with one barcode per record; apply the result with ``records[perm]`` and ``em.gather_names(x, perm)``.
    It turns ``add_umi_duplicates``' output into input for the collated UMI session.  A pure function of its argument."""
    blob, off = np.asarray(record_barcodes[0], dtype=np.uint8), np.asarray(record_barcodes[1], dtype=np.int64)
    raw = blob.tobytes()
    first = {}
    rank = np.fromiter((first.setdefault(raw[int(off[i]):int(off[i + 1])], len(first)) for i in range(len(off) - 1)),
                       dtype=np.int64, count=len(off) - 1)
    return np.argsort(rank, kind="stable")


def cut_cell_records(records, names, secondary, cell_rec_off, barcodes, cuts, unmapped_every: int = 0, umis=None):
    """``shuffle_cell_records``' barcode-collated input cut into batches for a barcoded session
    (``CellsStream(barcodes=True)``), every record with its cell's barcode.  ``barcodes``: one per cell
    (``make_barcodes``; a label may recur).  ``unmapped_every=k > 0`` first sprinkles in extra unmapped records, one
    in front of the records 0, k, 2k, ... of the input, each with an empty name and an empty barcode.  ``cuts`` are record
    positions of the stream that results (the sprinkled records counted), in any order and with repeats (a repeat gives
    an empty batch); 0 and the stream's length are implied.  A cut may fall inside a cell and inside a read.  Returns a
    list of ``(records, barcodes, names, secondary)``, ``barcodes`` and ``names`` as ``(blob, offsets)`` pairs with the
    offsets of each batch from 0.  With ``umis`` -- a ``(blob, offsets)`` pair, one UMI per record -- the tuples gain
    the batch's UMIs as a fifth element; a sprinkled record's UMI is empty.  A pure function of its arguments."""
    from .em import gather_names
    records = np.asarray(records)
    blob, off = np.asarray(names[0], dtype=np.uint8), np.asarray(names[1], dtype=np.int64)
    cell_rec_off = np.asarray(cell_rec_off, dtype=np.int64)
    n, n_cells = len(records), len(cell_rec_off) - 1
    if len(off) != n + 1 or int(cell_rec_off[-1]) != n or len(barcodes) != n_cells:
        raise ValueError("names need one entry per record, cell_rec_off must end at len(records), barcodes need one per cell")
    secondary = np.zeros(n, dtype=np.uint8) if secondary is None else np.asarray(secondary, dtype=np.uint8)
    if len(secondary) != n:
        raise ValueError("secondary must have one entry per record")
    enc = [b.encode() if isinstance(b, str) else bytes(b) for b in barcodes]
    cell_off = np.zeros(n_cells + 1, dtype=np.int64)
    np.cumsum([len(b) for b in enc], out=cell_off[1:])
    cell_of = np.repeat(np.arange(n_cells), np.diff(cell_rec_off))
    bc_blob, bc_off = gather_names((np.frombuffer(b"".join(enc), dtype=np.uint8), cell_off), cell_of)
    return _sprinkle_and_cut(records, blob, off, bc_blob, np.asarray(bc_off, dtype=np.int64), secondary, cuts, unmapped_every, umis)


def cut_interleaved_records(records, names, secondary, record_barcodes, cuts, unmapped_every: int = 0, umis=None):
    """``interleave_cells``' uncollated input cut into batches for an any-order barcoded session
    (``CellsStream(barcodes=True, collated=False)``), as ``cut_cell_records`` cuts collated input: ``record_barcodes`` is
    the ``(blob, offsets)`` pair with one barcode per record that ``interleave_cells`` returns; ``unmapped_every`` and
    ``cuts`` and ``umis`` mean what they mean there.  Returns a list of ``(records, barcodes, names, secondary)``, with
    ``umis`` of ``(records, barcodes, names, secondary, umis)``.  A pure function of its arguments."""
    records = np.asarray(records)
    blob, off = np.asarray(names[0], dtype=np.uint8), np.asarray(names[1], dtype=np.int64)
    bc_blob, bc_off = np.asarray(record_barcodes[0], dtype=np.uint8), np.asarray(record_barcodes[1], dtype=np.int64)
    n = len(records)
    if len(off) != n + 1 or len(bc_off) != n + 1:
        raise ValueError("names and record_barcodes need one entry per record")
    secondary = np.zeros(n, dtype=np.uint8) if secondary is None else np.asarray(secondary, dtype=np.uint8)
    if len(secondary) != n:
        raise ValueError("secondary must have one entry per record")
    return _sprinkle_and_cut(records, blob, off, bc_blob, bc_off, secondary, cuts, unmapped_every, umis)


def _sprinkle_and_cut(records, blob, off, bc_blob, bc_off, secondary, cuts, unmapped_every, umis=None):
    """the stream of ``cut_cell_records`` / ``cut_interleaved_records`` from one name and one barcode per record (and,
    with ``umis``, one UMI)"""
    from .builder import REC_UNMAPPED
    n = len(records)
    if umis is not None:
        u_blob, u_off = np.asarray(umis[0], dtype=np.uint8), np.asarray(umis[1], dtype=np.int64)
        if len(u_off) != n + 1:
            raise ValueError("umis need one entry per record")
    if unmapped_every > 0 and n:   # record i of the input goes to position i + i // k + 1
        pos = np.arange(n) + np.arange(n) // unmapped_every + 1
        total = int(pos[-1]) + 1
        stream = np.zeros(total, dtype=records.dtype)
        stream["flags"] = REC_UNMAPPED
        stream[pos] = records
        sec = np.zeros(total, dtype=np.uint8)
        sec[pos] = secondary
        name_len, bc_len = np.zeros(total, dtype=np.int64), np.zeros(total, dtype=np.int64)
        name_len[pos], bc_len[pos] = np.diff(off), np.diff(bc_off)
        off, bc_off = np.zeros(total + 1, dtype=np.int64), np.zeros(total + 1, dtype=np.int64)
        np.cumsum(name_len, out=off[1:])
        np.cumsum(bc_len, out=bc_off[1:])
        if umis is not None:
            umi_len = np.zeros(total, dtype=np.int64)
            umi_len[pos] = np.diff(u_off)
            u_blob, u_off = u_blob[int(u_off[0]):int(u_off[-1])], np.zeros(total + 1, dtype=np.int64)
            np.cumsum(umi_len, out=u_off[1:])
        records, secondary, n = stream, sec, total
    edges = [0] + sorted(int(c) for c in cuts) + [n]
    if edges[1] < 0 or edges[-2] > n:
        raise ValueError("a cut lies outside the records")
    out = []
    for a, b in zip(edges[:-1], edges[1:]):
        o, bo = off[a:b + 1], bc_off[a:b + 1]
        out.append((np.ascontiguousarray(records[a:b]),
                    (np.ascontiguousarray(bc_blob[int(bo[0]):int(bo[-1])]), np.ascontiguousarray(bo - bo[0], dtype=np.uint64)),
                    (np.ascontiguousarray(blob[int(o[0]):int(o[-1])]), np.ascontiguousarray(o - o[0], dtype=np.uint64)),
                    np.ascontiguousarray(secondary[a:b])))
        if umis is not None:
            uo = u_off[a:b + 1]
            out[-1] += ((np.ascontiguousarray(u_blob[int(uo[0]):int(uo[-1])]), np.ascontiguousarray(uo - uo[0], dtype=np.uint64)),)
    return out


@dataclass
class SyntheticProjectedRecords:
    filters: dict                # the fields of oem_filters the records were made for
    txp_len: np.ndarray          # u64 [T]
    records: np.ndarray          # builder.PROJ_RECORD [n_records]
    group_off: np.ndarray        # u64 [n_groups + 1]
    read_len: np.ndarray         # u64 [n_groups]
    beta: float                  # --projected-prob-beta the similarities were made for
    kept: np.ndarray             # u32 [n_groups]: what the filter keeps of each group
    discard: dict                # the discard table the filter ends with


def make_projected_records(store: SyntheticStore, seed: int = BASE_SEED + 22, decoy_rate: float = 0.3, drop_frac: float = 0.05,
                           score_prob_denom: float = 5.0) -> SyntheticProjectedRecords:
    """A synthetic store turned back into the projected (genome-mode) records it could have come from, so that
    AlignmentFilters::filter_projected (oarfish_types.rs:1179-1297) over them gives the store again: the same reads in
    the same order, the same transcripts, and -- under the default probability source, similarity -- the same
    ``as_prob``, in the spirit of ``make_records``.

    Each read gets a best similarity in [0.9, 1) and each kept alignment ``similarity = best + ln(p) / beta``, so that
    ``expf((float)(similarity - best) * beta)`` is its ``as_prob`` p again up to the f32 rounding of the argument
    (relative error about 1.2e-7 * (1 + |ln p|)).  ``beta`` is chosen from the store, at least 10, so that no kept
    similarity falls below 0.55 of its read's best; the score threshold is 0.5.  ``aln_score`` is ``best - g`` with g the
    integer gap of ``make_records``, so the score source reproduces ``expf(-g / D)`` as well.  Coordinates are 1-based
    and inside the transcripts (the clamp leaves them alone).  Per read, Poisson(``decoy_rate``) DECOY records are each
    rejected by exactly one test (orientation, aligned length, 3' clip, 5' clip in the first walk -- these carry a
    similarity above the read's best, which they must not become -- or the similarity threshold in the second); whole
    reads are dropped (``drop_frac`` of the groups) by a best similarity of 0, by a best alignment that covers a tenth
    of the read, or because the orientation test leaves nothing.  ``kept`` and ``discard`` are what the filter must
    report; discard_supp, no_mapping and no_valid_aln stay 0, filter_projected never counts them.  A pure function of
    (store, seed, rates, D)."""
    from .builder import PROJ_RECORD, REC_REVERSE
    F5, F3 = 2000, 3000
    filters = dict(five_prime_clip=F5, three_prime_clip=F3, score_threshold=0.5, min_aligned_fraction=0.5,
                   min_aligned_len=50, which_strand=1, score_prob_denom=float(score_prob_denom))
    rng = np.random.default_rng([seed, 0x9207EC])
    R, T, nnz = store.n_reads, store.n_txps, store.nnz
    rp = store.row_ptr.astype(np.int64)
    lens = np.diff(rp)
    if R and lens.min() < 1:
        raise ValueError("make_projected_records needs a store without empty reads")
    txp_len = rng.integers(400, 6000, size=T).astype(np.uint64)
    logp = np.log(store.as_prob.astype(np.float64))
    gap = np.rint(-float(score_prob_denom) * logp).astype(np.int64)
    first = rp[:-1]
    if R and np.maximum.reduceat(logp, first).min() != 0.0:
        raise ValueError("make_projected_records needs a read's best alignment to have as_prob 1")
    beta = float(max(10.0, np.ceil(2.5 * float(-logp.min())))) if nnz else 10.0
    best_sim = 0.9 + 0.1 * rng.random(R)
    best_score = rng.integers(1000, 3000, size=R)
    read_of = np.repeat(np.arange(R, dtype=np.int64), lens)
    # coordinates of the real alignments: 1 <= start < min(L - 100, F5), end in (max(start + 100, L - F3), L]
    L = txp_len[store.tid].astype(np.int64)
    start = 1 + (rng.random(nnz) * (np.minimum(L - 100, F5) - 1)).astype(np.int64)
    lo = np.maximum(start + 100, L - F3 + 1)
    end = np.minimum(lo + (rng.random(nnz) * (L - lo + 1)).astype(np.int64), L)
    span = end - start + 1
    # the read's length: the first best alignment covers more than half of it
    is_best = np.flatnonzero(logp == 0.0)
    _, where = np.unique(read_of[is_best], return_index=True)
    span_best = span[is_best[where]] if R else np.zeros(0, dtype=np.int64)
    rlen = span_best + (rng.random(R) * span_best).astype(np.int64)
    rlen = np.minimum(rlen, 2 * span_best - 1)

    # groups: the R reads in order, with dropped reads scattered between them
    n_drop = int(round(R * drop_frac / max(1e-9, 1.0 - drop_frac))) if R else 0
    G = R + n_drop
    is_real = np.ones(G, dtype=bool)
    if n_drop:
        is_real[rng.choice(G, size=n_drop, replace=False)] = False
    drop_kind = rng.integers(0, 3, size=n_drop)
    nd = rng.poisson(decoy_rate, size=R).astype(np.int64)
    nf = rng.binomial(nd, 0.5).astype(np.int64)                        # decoys in front of the real records
    n_rec = np.zeros(G, dtype=np.int64)
    n_rec[is_real] = lens + nd
    n_rec[~is_real] = np.where(drop_kind == 2, 2, 1)
    group_off = np.zeros(G + 1, dtype=np.uint64)
    np.cumsum(n_rec, out=group_off[1:])
    base_real = group_off[:-1][is_real].astype(np.int64)
    base_drop = group_off[:-1][~is_real].astype(np.int64)
    rec = np.zeros(int(group_off[-1]), dtype=PROJ_RECORD)
    read_len = np.zeros(G, dtype=np.uint64)
    read_len[is_real] = rlen
    read_len[~is_real] = 1000

    # the real records
    pos = np.repeat(base_real + nf, lens) + (np.arange(nnz, dtype=np.int64) - np.repeat(first, lens))
    rec["ref_id"][pos] = store.tid
    rec["start"][pos] = start
    rec["end"][pos] = end
    rec["aligned_len"][pos] = span
    rec["query_aligned_len"][pos] = span
    rec["similarity"][pos] = np.where(logp == 0.0, best_sim[read_of], best_sim[read_of] + logp / beta)
    rec["aln_score"][pos] = best_score[read_of] - gap

    # the decoys: kind 0 orientation, 1 aligned length, 2 3' clip, 3 5' clip, 4 similarity threshold
    n_dec = int(nd.sum())
    d_read = np.repeat(np.arange(R, dtype=np.int64), nd)
    q = np.arange(n_dec, dtype=np.int64) - np.repeat(np.cumsum(nd) - nd, nd)
    d_pos = base_real[d_read] + np.where(q < nf[d_read], q, lens[d_read] + q)
    d_tid = rng.integers(0, T, size=n_dec)
    d_L = txp_len[d_tid].astype(np.int64)
    kind = rng.integers(0, 5, size=n_dec)
    kind = np.where((kind == 2) & (d_L < F3), 0, kind)                 # (no 3' decoy on a transcript shorter than the clip)
    rec["ref_id"][d_pos] = d_tid
    rec["start"][d_pos] = np.where(kind == 3, F5, 1)
    rec["end"][d_pos] = np.where(kind == 2, d_L - F3, d_L)
    rec["aligned_len"][d_pos] = np.where(kind == 1, 10, 100)
    rec["query_aligned_len"][d_pos] = rlen[d_read]
    rec["similarity"][d_pos] = np.where(kind == 4, 0.3 * best_sim[d_read], best_sim[d_read] + 0.5)
    rec["aln_score"][d_pos] = np.where(kind == 4, best_score[d_read] - 1000, best_score[d_read] + 50)
    rec["flags"][d_pos] = np.where(kind == 0, REC_REVERSE, 0)

    # the dropped reads: 0 = best similarity 0 (no counter moves), 1 = the best alignment covers a tenth of the read,
    # 2 = two reverse-strand records, so that nothing is retained
    for k in range(3):
        b = base_drop[drop_kind == k]
        for j in range(2 if k == 2 else 1):
            t = rng.integers(0, T, size=len(b))
            rec["ref_id"][b + j] = t
            rec["start"][b + j] = 1
            rec["end"][b + j] = txp_len[t]
            rec["aligned_len"][b + j] = 100
            rec["query_aligned_len"][b + j] = 100
            rec["similarity"][b + j] = 0.0 if k == 0 else 0.95
            rec["aln_score"][b + j] = 500
            rec["flags"][b + j] = REC_REVERSE if k == 2 else 0
    kept = np.zeros(G, dtype=np.uint32)
    kept[is_real] = lens
    discard = dict(discard_5p=int((kind == 3).sum()), discard_3p=int((kind == 2).sum()), discard_score=int((kind == 4).sum()),
                   discard_aln_frac=int((drop_kind == 1).sum()), discard_aln_len=int((kind == 1).sum()),
                   discard_ori=int((kind == 0).sum()) + 2 * int((drop_kind == 2).sum()), discard_supp=0, valid_best_aln=R,
                   no_mapping=0, no_valid_aln=0)
    return SyntheticProjectedRecords(filters, txp_len, rec, group_off, read_len, beta, kept, discard)


def cut_projected_records(spr, sizes):
    """``make_projected_records``' output cut at group boundaries into batches for a projected session
    (``RecordsStream(projected=True)``): ``sizes`` are numbers of groups, in input order; a size 0 gives an empty batch,
    and the groups the sizes leave over form a last batch (also when none are left and ``sizes`` is empty).  ``spr`` is
    a ``SyntheticProjectedRecords`` or a ``(records, group_off, read_len)`` triple.  Returns a list of ``(records,
    group_off, read_len)``, each batch's ``group_off`` from 0.  A pure function of its arguments."""
    records, group_off, read_len = (spr.records, spr.group_off, spr.read_len) if hasattr(spr, "group_off") else spr
    records = np.asarray(records)
    group_off, read_len = np.asarray(group_off, dtype=np.uint64), np.asarray(read_len, dtype=np.uint64)
    n_groups = len(group_off) - 1
    sizes = [int(s) for s in sizes]
    if any(s < 0 for s in sizes) or sum(sizes) > n_groups:
        raise ValueError("the sizes must be non-negative and sum to at most the number of groups")
    if sum(sizes) < n_groups or not sizes:
        sizes = sizes + [n_groups - sum(sizes)]
    out, g0 = [], 0
    for s in sizes:
        o = group_off[g0:g0 + s + 1]
        out.append((np.ascontiguousarray(records[int(o[0]):int(o[-1])]), np.ascontiguousarray(o - o[0]),
                    np.ascontiguousarray(read_len[g0:g0 + s])))
        g0 += s
    return out


def cell_shift(rep: int, n_txps: int) -> int:
    """Transcript-id rotation of replica ``rep`` of a cell in ``replicate_cells``."""
    return (rep * 7919) % n_txps


def replicate_cells(cells, n_txps: int, n_cells: int):
    """BASELINE configs[4] whole (5 k cells x 50 k reads, 2 G alignments) without generating 5 k cells in Python
    (~0.1 s of one core per cell): ``cells`` = (cell_off, row_ptr, tid, as_prob) of n_base generated cells, and cell
    ``r * n_base + c`` of the result is cell c with every transcript id rotated by ``cell_shift(r, n_txps)``
    (t -> (t + shift) mod T).  A relabelling of the transcripts is an exact symmetry of the EM, so the copies are
    distinct problems for the engine (other ids, other tiles, other windows) whose answers are known in terms of each
    other: counts[r * n_base + c][(t + shift) mod T] == counts[c][t] up to summation order."""
    cell_off_b, row_ptr_b, tid_b, p_b = cells
    n_base = len(cell_off_b) - 1
    reps = -(-n_cells // n_base)
    nnz_b, reads_b = len(tid_b), len(row_ptr_b) - 1
    tid = np.empty(nnz_b * reps, dtype=np.uint32)
    for r in range(reps):
        seg = tid[r * nnz_b:(r + 1) * nnz_b]
        np.add(tid_b, np.uint32(cell_shift(r, n_txps)), out=seg)
        np.subtract(seg, np.uint32(n_txps), out=seg, where=seg >= n_txps)
    row_ptr = np.empty(reads_b * reps + 1, dtype=np.uint64)
    cell_off = np.empty(n_base * reps + 1, dtype=np.uint64)
    for r in range(reps):
        row_ptr[r * reads_b:(r + 1) * reads_b] = row_ptr_b[:-1] + np.uint64(r * nnz_b)
        cell_off[r * n_base:(r + 1) * n_base] = np.asarray(cell_off_b[:-1], dtype=np.uint64) + np.uint64(r * reads_b)
    row_ptr[-1] = np.uint64(reps * nnz_b)
    cell_off[-1] = np.uint64(reps * reads_b)
    p = np.tile(p_b, reps)
    if n_cells < n_base * reps:   # trim to whole cells
        r1 = int(cell_off[n_cells])
        a1 = int(row_ptr[r1])
        return cell_off[:n_cells + 1].copy(), row_ptr[:r1 + 1].copy(), tid[:a1].copy(), p[:a1].copy()
    return cell_off, row_ptr, tid, p


def make_sirv_store(tag: str = "C", n_reads: int = 20_000, seed: int = BASE_SEED + 1,
                    coverage: bool = False, table_path: Optional[str] = None) -> SyntheticStore:
    """BASELINE config[0] stand-in: a SIRV-shaped store (T = 69 / 44 / 100 for the C / I / O
    annotations).  The reference's test_data has no BAM or reads, so reads are synthesised over
    the real SIRV isoform structure (tests/golden/sirv_txps.json: gene, length and pairwise exonic
    overlap of every transcript, derived from the reference's GTFs by scripts/make_sirv_fixture.py):
    a read's primary is drawn from a log-normal mix; every isoform of the same gene that shares
    exonic sequence with it is a secondary alignment with probability overlap/length, scored with
    a deficit that grows as the overlap shrinks."""
    import json
    import os
    if table_path is None:
        table_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                  "tests", "golden", "sirv_txps.json")
    tab = json.load(open(table_path))[tag]
    T = len(tab["names"])
    length = np.asarray(tab["length"], dtype=np.float64)
    ov = np.zeros((T, T))
    for k, v in tab["overlap"].items():
        i, j = (int(x) for x in k.split(","))
        ov[i, j] = ov[j, i] = v
    rng = np.random.default_rng([seed, ord(tag)])
    a = rng.lognormal(0.0, 1.5, size=T)
    a /= a.sum()
    t0 = rng.choice(T, size=n_reads, p=a)
    frac = np.clip(ov[t0] / length[t0][:, None], 0.0, 1.0)         # [n_reads, T]
    take = rng.random((n_reads, T)) < frac
    take[np.arange(n_reads), t0] = True
    d = np.minimum(np.floor((1.0 - frac) * 12.0) + rng.geometric(0.3, size=(n_reads, T)) - 1, 60)
    d[np.arange(n_reads), t0] = 0
    rows, cols = np.nonzero(take)
    p = np.exp((-d[rows, cols].astype(np.float32)) / np.float32(5.0)).astype(np.float32)
    lens = np.bincount(rows, minlength=n_reads).astype(np.uint64)
    row_ptr = np.zeros(n_reads + 1, dtype=np.uint64)
    np.cumsum(lens, out=row_ptr[1:])
    cov = None
    if coverage:
        cov = rng.uniform(0.05, 1.0, size=len(cols))
        ssum = np.add.reduceat(cov, row_ptr[:-1].astype(np.int64))
        cov = cov / np.repeat(ssum, lens.astype(np.int64))
    return SyntheticStore(row_ptr, cols.astype(np.uint32), p, cov, T, a, np.asarray(tab["gene"], dtype=np.int32))
