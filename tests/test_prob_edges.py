"""CPU test of the expected side of the `.prob` edge cases (tests/prob_edges_common.py): the store is exact in
rationals, and the oracle's probabilities printed by Python say, at every threshold, what the cases claim -- the ties
land on the even neighbour, a probability equal to the threshold is kept and its upper neighbour keeps nothing, the
-0.0 is printed with its sign, 1 - 2^-32 carries into `1.000000000`.  tests/test_assignment_text_gpu.py holds the
device to the same text."""
import numpy as np
import pytest

from oarfish_amd import writers
from oracle import c_oracle

from . import prob_edges_common as pe


@pytest.fixture(scope="module")
def st():
    return pe.EdgeStore()


def test_the_edge_store_is_exact_and_spans_workgroups(st):
    pe.assert_exact(st)
    assert st.n_reads >= 600 and st.n_reads > 2 * 256
    assert {len(str(int(t))) for t in st.tid} == {1, 2, 3}
    assert 1.0 / 5.0 == 0.2 and 1.0 / 4.0 == 0.25 and 1.0 / 2.0 == 0.5
    assert [writers.prob_display_decimals(pe.tie_thresh(k)) for k in pe.TIE_KS] == [3, 4, 5, 6, 7, 8, 9]
    assert len(set(pe.THRESHOLDS)) == len(pe.THRESHOLDS) == 17


@pytest.mark.parametrize("thresh", pe.THRESHOLDS, ids=repr)
def test_the_oracle_text_says_what_the_cases_claim(st, thresh):
    o = c_oracle.Store(st.row_ptr, st.tid, st.as_prob, None, st.n_txps)
    probs = c_oracle.assignment_probs(o, st.counts, thresh)
    body, line_off, kept = pe.expected_text(st, probs, thresh, st.names)
    pe.check_edge_lines(st, thresh, body, line_off, kept)
    assert np.array_equal(kept, np.add.reduceat((probs >= 0).astype(np.int64), st.row_ptr[:-1].astype(np.int64)))
    if thresh == 0.0:
        assert kept.sum() == len(st.tid) and np.signbit(probs[st.row(st.read("zero"))][0])


def test_python_formatting_is_half_even_on_the_printed_values(st):
    """`f"{x:.{d}f}"`, the formatting the expected text is made with, against the rounding worked out in rationals,
    on every probability the oracle hands out for the edge store."""
    o = c_oracle.Store(st.row_ptr, st.tid, st.as_prob, None, st.n_txps)
    n = 0
    for thresh in pe.THRESHOLDS:
        d = writers.prob_display_decimals(thresh)
        probs = c_oracle.assignment_probs(o, st.counts, thresh)[:int(st.row_ptr[len(pe.BLOCK_READS)])]   # one block
        for x in probs[probs >= 0]:
            assert f"{abs(float(x)):.{d}f}" == pe.half_even(abs(float(x)), d), (thresh, x)
            n += 1
    assert n > 300
