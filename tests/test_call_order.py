"""CPU tier of the call-order tests (tests/call_order_common.py): the walk really visits every ordered pair, the
alphabet and the named pairs are well-formed, and the inputs keep every converging run of the alphabet off the
stopping rule's knife-edge -- the GPU tier requires niter, n_passes and converged to be EXACTLY those of a fresh
handle and of the oracle, which only means something where a rel_diff within the noise of THRESH cannot flip them."""
import itertools

import pytest

from tests import call_order_common as co


@pytest.mark.parametrize("n", [1, 2, 5, 21, len(co.OPS)])
def test_euler_walk_has_every_ordered_pair_exactly_once(n):
    w = co.euler_walk(n)
    assert len(w) == n * n + 1 and w[0] == w[-1] == 0
    pairs = list(zip(w, w[1:]))
    assert len(set(pairs)) == len(pairs) == n * n
    assert set(pairs) == set(itertools.product(range(n), repeat=2))


def test_alphabet_names_are_unique_and_pairs_name_known_operations():
    names = [op.name for op in co.OPS]
    assert len(set(names)) == len(names) >= 21
    assert all(op.kind in ("pass", "run40", "converged", "exact", "state") for op in co.OPS)
    assert co.PAIRS and all(a in co.BY_NAME and b in co.BY_NAME for a, b in co.PAIRS)
    assert len(set(co.PAIRS)) == len(co.PAIRS)
    assert {op.name for op in co.KNOB_FREE} == set(names) - {"em_40_classic", "em_converged_graph", "boot_batched",
                                                            "boot_byte_edge", "history_500"}


@pytest.mark.parametrize("store", co.STORES)
def test_converging_runs_stop_off_the_knife_edge(store):
    """The point estimate and every replicate that runs under THRESH: converged between the gate and max_iter, with the
    rel_diff of the stopping iteration and of the one before at least MARGIN * THRESH away from THRESH (a replicate
    the gate stops, with both values far below THRESH, is as safe as one the threshold stops)."""
    rows = co.stopping_margins(store)
    assert len(rows) == 1 + 5 + 7 + co.N_DRAWN + 6
    for what, niter, conv, rel_last, rel_prev in rows:
        print(f"store {store}: {what}: niter {niter}, margins {abs(rel_last - co.THRESH) / co.THRESH:.2e} (stop) "
              f"{abs(rel_prev - co.THRESH) / co.THRESH:.2e} (before)")
    for what, niter, conv, rel_last, rel_prev in rows:
        assert conv and co.GATE < niter < co.MAX_ITER, (store, what, niter, conv)
        assert rel_last < co.THRESH, (store, what, rel_last)
        assert abs(rel_last - co.THRESH) >= co.MARGIN * co.THRESH, (store, what, rel_last)
        assert abs(rel_prev - co.THRESH) >= co.MARGIN * co.THRESH, (store, what, rel_prev)
