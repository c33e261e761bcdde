"""The edge grid of the coverage model, shared by test_coverage_edges.py (oracle and host restatement, no GPU) and
test_coverage_edges_gpu.py (the whole-store kernels of oem_coverage_device.hip and the per-cell ones of
oem_coverage_cells.hip).

A geometry is one (transcript length, bin width) pair.  Its alignments are every ordered pair of the points
around its bin edges -- the edges of the requested width W (normalize_read_probs), of the rounded width
round(L / n) (add_interval's bins) and of the exact width L / n (add_interval's start_bin / end_bin) -- plus one
zero span, one start > end and one alignment that ends one base past the transcript.  Every alignment is a read of
two: itself on the geometry's transcript and a fixed partner (10, 700) on the geometry's own 777-base transcript.
The bin width is one argument of a coverage call, so stores and cell layouts are built per width.
"""
import functools
import math

import numpy as np

from oracle import filter_py as fp

GEOMETRIES = [(1, 1), (1, 100), (2, 1), (3, 2), (5, 3), (50, 100), (99, 100), (100, 100), (101, 100), (150, 100),
              (199, 100), (200, 100), (201, 100), (250, 100), (1000, 100), (1001, 100), (1050, 100), (10050, 100),
              (10140, 100), (64, 64), (128, 64), (4096, 64), (4096, 4096), (4097, 4096), (777, 7), (6000, 1),
              (2 ** 24 + 1, 2 ** 23), (4_000_000_000, 2 ** 30)]
WIDTHS = sorted({w for _, w in GEOMETRIES})
# overlap fractions that are dyadic: the bins are exact in any summation order
POW2_GEOMETRIES = [(64, 64), (128, 64), (4096, 64), (4096, 4096)]
PARTNER_LEN, PARTNER = 777, (10, 700)
MODELS = {"logistic": 0, "binomial": 1}
GROWTH = 2.0
# r = 1 / (1 + exp(-a * diff)), diff = (expected - count) / expected <= 1: the upper clamp 0.99999 needs
# a * diff > 11.6 and the lower clamp 1e-8 needs a * diff < -18.5.  With a = 64 a bin at 0.8 of the mean or below
# and one at 1.3 of the mean or above reach them (test_coverage_edges.py asserts that both occur).
GROWTH_LARGE = 64.0
ZERO, REVERSED, PAST_END, PLAIN = "zero span", "start > end", "one past the end", "plain"


def n_bins(L, W):
    return int(math.ceil(float(L) / float(W)))                     # with_len_and_bin_width (oarfish_types.rs:464)


def rounded_width(L, W):
    return fp._rust_round(float(L) / float(n_bins(L, W)))          # add_interval (:501)


def points(L, W):
    n, bw = n_bins(L, W), rounded_width(L, W)
    pts = {0, 1, L // 2, L - 1, L}
    edges = set()
    for b in range(1, min(n, 4) + 1):
        edges |= {b * W, int(b * bw), int(b * L / n)}
    edges |= {(n - 1) * W, int((n - 1) * bw)}
    for g in edges:
        pts |= {g - 1, g, g + 1}
    return sorted(p for p in pts if 0 <= p <= L)


def end_bin_of_add_interval(stop, L, W):
    return int(math.floor((float(stop) / float(L)) * float(n_bins(L, W))))      # :505


def past_end_is_a_value(L, W):
    """stop = L + 1 is inside add_interval's slice [start_bin..end_bin] while end_bin == n."""
    return end_bin_of_add_interval(L + 1, L, W) == n_bins(L, W)


def alignments(L, W):
    """[(start, end, kind)] of one geometry."""
    pts = points(L, W)
    out = [(s, e, PLAIN) for s in pts for e in pts if s < e]
    mid = pts[len(pts) // 2]
    out.append((mid, mid, ZERO))
    out.append((pts[-1], pts[0], REVERSED))
    if past_end_is_a_value(L, W):
        out.append((L // 2, L + 1, PAST_END))
    return out


class Grid:
    """Reads over 2 transcripts per geometry (transcript 2 g: the geometry's, 2 g + 1: its partner's), as arrays for
    the library and as the oracle's fp.Store.  geom[r], kind[r]: the geometry and the kind of read r."""

    def __init__(self, geoms, reads):
        self.geoms = list(geoms)
        self.txp_len = [x for L, _ in self.geoms for x in (L, PARTNER_LEN)]
        self.tl = np.asarray(self.txp_len, dtype=np.uint64)
        self.geom = [g for g, _, _, _ in reads]
        self.kind = [k for _, _, _, k in reads]
        n = len(reads)
        self.row_ptr = (2 * np.arange(n + 1)).astype(np.uint64)
        self.tid = np.asarray([t for g, _, _, _ in reads for t in (2 * g, 2 * g + 1)], dtype=np.uint32)
        self.start = np.asarray([x for _, s, _, _ in reads for x in (s, PARTNER[0])], dtype=np.uint32)
        self.end = np.asarray([x for _, _, e, _ in reads for x in (e, PARTNER[1])], dtype=np.uint32)
        self.as_prob = np.tile(np.asarray([0.8, 1.0], dtype=np.float32), n)
        self.n_reads, self.nnz, self.n_txps = n, 2 * n, len(self.txp_len)

    def fp_store(self, order=None):
        """The oracle's twin; `order`: a permutation of the reads (the store order add_interval sums in)."""
        order = range(self.n_reads) if order is None else order
        st = fp.Store()
        for r in order:
            for j in (2 * r, 2 * r + 1):
                st.tid.append(int(self.tid[j])); st.start.append(int(self.start[j])); st.end.append(int(self.end[j]))
            st.row_ptr.append(len(st.tid))
        return st

    def reads_of(self, g):
        return np.asarray([r for r in range(self.n_reads) if self.geom[r] == g], dtype=np.int64)


def geometries_of(width):
    return [(L, W) for L, W in GEOMETRIES if W == width]


@functools.lru_cache(maxsize=None)
def store(width):
    """Every geometry of one bin width in one store."""
    geoms = geometries_of(width)
    return Grid(geoms, [(g, s, e, k) for g, (L, W) in enumerate(geoms) for s, e, k in alignments(L, W)])


@functools.lru_cache(maxsize=None)
def oracle(width, model, growth):
    """filter_py.coverage_probs on store(width), computed once (read-only)."""
    g = store(width)
    out = np.asarray(fp.coverage_probs(g.fp_store(), g.txp_len, width, growth, model=model))
    out.setflags(write=False)
    return out


class Cells:
    """store(width) cut into cells over the same annotation: one cell per geometry, an empty cell after the first
    one, and a last cell that reuses the transcripts of the geometry with the most bins with different alignments:
    the first third of that geometry's reads (`n_shared`, the reads the pair can be compared on) and then eight
    copies of an alignment over the first bin only.  Two coverages of one transcript: the bins must be per cell."""

    def __init__(self, width):
        whole = store(width)
        self.width, self.geoms = width, whole.geoms
        self.reused = max(range(len(self.geoms)), key=lambda g: n_bins(*self.geoms[g]))
        read = lambda r: (whole.geom[r], int(whole.start[2 * r]), int(whole.end[2 * r]), whole.kind[r])  # noqa: E731
        cells = [[read(r) for r in whole.reads_of(g)] for g in range(len(self.geoms))]
        self.first_of_pair = self.reused + (1 if self.reused >= 1 else 0)
        self.empty_cell = 1
        cells.insert(self.empty_cell, [])
        L, W = self.geoms[self.reused]
        own = cells[self.first_of_pair]
        self.n_shared = max(len(own) // 3, 2)
        cells.append(own[:self.n_shared] + [(self.reused, 0, L // n_bins(L, W) + 1, PLAIN)] * 8)
        self.second_of_pair = len(cells) - 1
        self.grid = Grid(self.geoms, [x for c in cells for x in c])
        self.cell_off = np.concatenate([[0], np.cumsum([len(c) for c in cells])]).astype(np.uint64)
        self.n_cells = len(cells)

    def pair_can_differ(self, model):
        """Two binomial bins get 0.5 each whatever their counts (pmf(m; S, p) == pmf(S - m; S, 1 - p)), so a reused
        transcript of two bins tells the two coverages apart under the logistic model only."""
        return model == "logistic" or n_bins(*self.geoms[self.reused]) >= 3

    def pair_columns(self, col):
        """The values in `col` of the reads the two cells of the pair share: (first cell's, reusing cell's)."""
        a0, b0 = self.read_range(self.first_of_pair)[0], self.read_range(self.second_of_pair)[0]
        k = np.arange(self.n_shared)
        ia, ib = np.concatenate([2 * (a0 + k), 2 * (a0 + k) + 1]), np.concatenate([2 * (b0 + k), 2 * (b0 + k) + 1])
        assert np.array_equal(self.grid.start[ia], self.grid.start[ib]) and np.array_equal(self.grid.end[ia], self.grid.end[ib])
        return np.asarray(col)[ia], np.asarray(col)[ib]

    def read_range(self, c):
        return int(self.cell_off[c]), int(self.cell_off[c + 1])

    def cell_store(self, c):
        r0, r1 = self.read_range(c)
        return self.grid.fp_store(range(r0, r1))


@functools.lru_cache(maxsize=None)
def cells(width):
    return Cells(width)


@functools.lru_cache(maxsize=None)
def cells_oracle(width, model, growth):
    """filter_py.coverage_probs on each cell's own store, concatenated (read-only)."""
    cl = cells(width)
    out = np.zeros(cl.grid.nnz)
    for c in range(cl.n_cells):
        r0, r1 = cl.read_range(c)
        if r1 > r0:
            out[2 * r0:2 * r1] = fp.coverage_probs(cl.cell_store(c), cl.grid.txp_len, width, growth, model=model)
    out.setflags(write=False)
    return out


def rel_err(got, want):
    """Relative error on the finite entries of `want`, after asserting NaN in exactly the same places."""
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN positions differ from the oracle's"
    fin = ~np.isnan(want)
    assert np.all(np.isfinite(got[fin]))
    return np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-300), fin


def assert_device_close(got, want, model, what, exact_reads=None):
    """The bounds of test_cells_coverage_gpu._assert_close against the oracle: NaN positions equal, rtol 2e-6, median
    relative error 1e-12 (logistic) or 1e-9 (binomial).  exact_reads: reads whose bins are exact in any order (the
    power-of-two geometries); under the logistic model their maximum relative error is 1e-12."""
    rel, fin = rel_err(got, want)
    med = 1e-12 if model == "logistic" else 1e-9
    print(f"{what}: n={fin.sum()} nan={(~fin).sum()} max rel={rel.max():.3e} median rel={np.median(rel):.3e}")
    np.testing.assert_allclose(np.asarray(got)[fin], np.asarray(want)[fin], rtol=2e-6, atol=1e-300, err_msg=what)
    assert np.median(rel) <= med, (what, np.median(rel))
    if exact_reads is not None and model == "logistic" and len(exact_reads):
        idx = np.concatenate([2 * exact_reads, 2 * exact_reads + 1])
        full = np.full(len(want), np.nan)
        full[fin] = rel
        worst = np.nanmax(full[idx])
        print(f"{what}: power-of-two geometries max rel={worst:.3e}")
        assert worst <= 1e-12, (what, worst)


def pow2_reads(grid):
    gs = [g for g, geom in enumerate(grid.geoms) if geom in POW2_GEOMETRIES]
    return np.asarray([r for r in range(grid.n_reads) if grid.geom[r] in gs], dtype=np.int64)
