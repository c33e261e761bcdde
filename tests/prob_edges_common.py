"""A hand-made store whose `.prob` lines sit on the edges of the printing: exact rounding ties at every decimal count,
probabilities equal to the display threshold, a kept -0.0 and the carry into the integer digit.  Shared by
tests/test_prob_edges.py (the oracle and Python's formatting alone: the expected side, checked without a device) and
tests/test_assignment_text_gpu.py (the device).

Every product counts[t] * w and every partial sum of a read's denom is exactly representable (`assert_exact`, in
rationals), so a fused multiply-add on the device and its absence in the oracle cannot differ by a bit, and the
device's probabilities must equal the oracle's bit for bit.

A block of 13 reads over 9 transcripts, repeated REPEATS times with its transcript ids shifted (id lengths 1 .. 3,
more than two workgroups of reads).  The counts of a block's transcripts are BLOCK_COUNTS; its reads:

  tie4 .. tie10   weights (2^-k, 1 - 2^-k) on two counts of 1: denom 1, so the two probabilities are the weights.  At
                  d = k - 1 decimals (display_thresh 10^-(k-1)) both are exact ties: 2^-k * 10^(k-1) * 2 = 5^(k-1), odd.
  three           (3/16, 7/16, 6/16): `0.188 0.438 0.375` at d = 3, two ties that round up to even
  five, four, two n equal alignments: every probability is 1/n, which is the double 0.2, 0.25, 0.5
  zero            counts (-0.0, 3): the first probability is -0.0, kept at display_thresh 0 and printed with its sign
  carry           counts (1 - 2^-32, 2^-32): 0.99999999977 prints as 1.000000000"""
from fractions import Fraction

import numpy as np

from oarfish_amd import writers

REPEATS = 47
TIE_KS = tuple(range(4, 11))
BLOCK_COUNTS = (1.0, 1.0, 1.0, 1.0, 1.0, -0.0, 3.0, 1.0 - 2.0 ** -32, 2.0 ** -32)
BLOCK_READS = tuple([(f"tie{k}", (0, 1), (2.0 ** -k, 1.0 - 2.0 ** -k)) for k in TIE_KS] + [
    ("three", (0, 1, 2), (3 / 16, 7 / 16, 6 / 16)),
    ("five", (0, 1, 2, 3, 4), (1.0,) * 5),
    ("four", (0, 1, 2, 3), (1.0,) * 4),
    ("two", (0, 1), (1.0,) * 2),
    ("zero", (5, 6), (1.0, 1.0)),
    ("carry", (7, 8), (1.0, 1.0)),
])
READ_AT = {name: i for i, (name, _, _) in enumerate(BLOCK_READS)}     # the read's index within its block
EQUAL_READS = (("five", 5, 0.2), ("four", 4, 0.25), ("two", 2, 0.5))


def tie_thresh(k: int) -> float:
    """The display_thresh at which tie<k> prints with k - 1 decimals."""
    return float(f"1e-{k - 1}")


def around(x: float) -> tuple:
    """(just below, x, just above)"""
    return float(np.nextafter(x, 0.0)), x, float(np.nextafter(x, 1.0))


# every threshold the edge store is run at: d = 3 .. 9, the three equalities with their neighbours, and 0
THRESHOLDS = tuple(tie_thresh(k) for k in TIE_KS) + tuple(t for _, _, p in EQUAL_READS for t in around(p)) + (0.0,)


class EdgeStore:
    def __init__(self, repeats: int = REPEATS):
        rows, w, names = [], [], []
        for rep in range(repeats):
            for name, ids, weights in BLOCK_READS:
                rows.append(np.asarray(ids, dtype=np.uint32) + np.uint32(rep * len(BLOCK_COUNTS)))
                w.append(weights)
                names.append(f"{name}/{rep}")
        self.n_reads = len(rows)
        self.n_txps = repeats * len(BLOCK_COUNTS)
        self.row_ptr = np.zeros(self.n_reads + 1, dtype=np.uint64)
        np.cumsum([len(r) for r in rows], out=self.row_ptr[1:])
        self.tid = np.concatenate(rows).astype(np.uint32)
        w64 = np.concatenate(w).astype(np.float64)
        self.as_prob = w64.astype(np.float32)
        assert np.array_equal(self.as_prob.astype(np.float64), w64)       # every weight is an f32
        self.counts = np.tile(np.array(BLOCK_COUNTS, dtype=np.float64), repeats)
        self.names = names

    def read(self, name: str, rep: int = 0) -> int:
        return rep * len(BLOCK_READS) + READ_AT[name]

    def row(self, r: int) -> slice:
        return slice(int(self.row_ptr[r]), int(self.row_ptr[r + 1]))


def assert_exact(st: EdgeStore) -> None:
    """In rationals: every product counts[t] * w and every partial sum of every read's denom is the double that f64
    arithmetic makes of it, with or without a fused multiply-add."""
    for r in range(st.n_reads):
        denom, exact = 0.0, Fraction(0)
        for j in range(int(st.row_ptr[r]), int(st.row_ptr[r + 1])):
            c, w = float(st.counts[st.tid[j]]), float(st.as_prob[j])
            assert Fraction(c * w) == Fraction(c) * Fraction(w), (r, j)
            exact += Fraction(c) * Fraction(w)
            denom += c * w
            assert Fraction(denom) == exact, (r, j)
        assert denom > 0.0 and denom == int(denom)                        # (1, 2, 3, 4 or 5)


def is_tie(x: float, d: int) -> bool:
    """x lies exactly half way between two d-decimal numbers."""
    v = Fraction(x) * 10 ** d * 2
    return v.denominator == 1 and v.numerator % 2 == 1


def half_even(x: float, d: int) -> str:
    """`{:.d}` of a finite x >= 0 worked out in rationals: the exact value rounded to d decimals, ties to even."""
    v = Fraction(x) * 10 ** d
    q, rem = divmod(v.numerator, v.denominator)
    if 2 * rem > v.denominator or (2 * rem == v.denominator and q % 2 == 1):
        q += 1
    return f"{q // 10 ** d}.{q % 10 ** d:0{d}d}"


def expected_text(st: EdgeStore, probs, thresh: float, names=None):
    """(body, line_off, kept) of the `.prob` body from the oracle's probabilities (-1: not printed), with Python's
    `f"{x:.{d}f}"` and `writers.prob_display_decimals` (write_function.rs:320-331)."""
    d = writers.prob_display_decimals(thresh)
    lines, kept = [], []
    for r in range(st.n_reads):
        p, ids = probs[st.row(r)], st.tid[st.row(r)]
        keep = p >= 0.0                                                   # (true for a kept -0.0)
        kept.append(int(keep.sum()))
        name = names[r] if names is not None else ""
        lines.append(f"{name}\t{kept[-1]}\t" + "\t".join(str(int(t)) for t in ids[keep]) + "\t"
                     + "\t".join(f"{float(x):.{d}f}" for x in p[keep]) + "\n")
    body = "".join(lines).encode()
    line_off = np.zeros(st.n_reads + 1, dtype=np.uint64)
    np.cumsum([len(l.encode()) for l in lines], out=line_off[1:])
    return body, line_off, np.array(kept, dtype=np.uint32)


def check_edge_lines(st: EdgeStore, thresh: float, body: bytes, line_off, kept) -> None:
    """What the lines of the edge reads must say at `thresh`, written out: on the expected text (is the case what
    it claims to be?) and on the device's (does the device print it?).  Every repeat of the block is checked."""
    d = writers.prob_display_decimals(thresh)
    lines = body.split(b"\n")
    assert lines[-1] == b"" and len(lines) == st.n_reads + 1
    assert np.array_equal(np.asarray(line_off[1:], dtype=np.int64), np.cumsum([len(l) + 1 for l in lines[:-1]]))

    def probs_of(r):
        f = lines[r].split(b"\t")
        k = int(f[1])
        assert k == kept[r] and f[0] == st.names[r].encode()
        return [x.decode() for x in f[2 + k:]] if k else []

    for rep in range(st.n_reads // len(BLOCK_READS)):
        for k in TIE_KS:
            if thresh == tie_thresh(k):
                lo, hi = 2.0 ** -k, 1.0 - 2.0 ** -k
                assert d == k - 1 and is_tie(lo, d) and is_tie(hi, d)
                got = probs_of(st.read(f"tie{k}", rep))
                assert got == [half_even(lo, d), half_even(hi, d)], (k, got)
                assert int(got[0][-1]) % 2 == 0 and int(got[1][-1]) % 2 == 0      # both landed on the even neighbour
                assert Fraction(got[0]) < Fraction(lo) and Fraction(got[1]) > Fraction(hi)   # one went down, one up
                if k == 4:
                    assert got == ["0.062", "0.938"]
                if k == 10:
                    assert got == ["0.000976562", "0.999023438"]
        if thresh == 1e-3:
            assert is_tie(3 / 16, 3) and is_tie(7 / 16, 3)
            assert probs_of(st.read("three", rep)) == ["0.188", "0.438", "0.375"]
        for name, n, p in EQUAL_READS:
            below, at, above = around(p)
            r = st.read(name, rep)
            if thresh in (below, at):
                assert kept[r] == n and probs_of(r) == [half_even(p, 3)] * n
            if thresh == above:
                assert kept[r] == 0 and lines[r] == st.names[r].encode() + b"\t0\t\t"
        if thresh == 0.0:
            r = st.read("zero", rep)
            assert kept[r] == 2 and lines[r].endswith(b"\t-0.000000000\t1.000000000")
            ids = st.tid[st.row(r)]
            assert int(line_off[r + 1] - line_off[r]) == len(st.names[r]) + 3 + sum(len(str(int(t))) + 1 for t in ids) + 12 + 1 + 11 + 1
            assert probs_of(st.read("carry", rep)) == ["1.000000000", "0.000000000"]
        elif thresh > 0.0:
            r = st.read("zero", rep)                                              # -0.0 >= thresh fails: one kept
            assert kept[r] == 1 and probs_of(r) == [half_even(1.0, d)]
