"""CPU test of the EM loop's stopping rule (oarfish_amd/csrc/oem_stopping_rule.h): the header's pure layer -- the
functions every loop kernel calls -- is compiled as host code and held to a transcription of the reference's loop
(src/em.rs:181, :194-201, :212-218) at the edges of every comparison."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "stopping_rule_shim.cpp")
LIB = os.path.join(HERE, "native", "libstopping_rule_shim.so")
U32 = 2**32 - 1


@pytest.fixture(scope="module")
def shim():
    hdr = os.path.join(HERE, "..", "oarfish_amd", "csrc", "oem_stopping_rule.h")
    abi = os.path.join(HERE, "..", "include", "oarfish_em.h")
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(map(os.path.getmtime, (SRC, hdr, abi))):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", LIB, SRC])
    L = C.CDLL(LIB)
    L.shim_stopping_rule.argtypes = [C.c_uint32, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double,
                                     C.POINTER(C.c_uint32 * 4)]
    L.shim_stopping_rule.restype = None
    L.shim_rel_diff_term.argtypes = [C.c_double] * 3
    L.shim_rel_diff_term.restype = C.c_double
    return L


def reference_step(niter, rel_diff, convergence_thresh, gate, max_iter):
    """One trip of do_em's loop from the comparison on: (niter, loop ends, left through `break`).  `gate` is the
    literal 50 of em.rs:212; niter is a u32."""
    if (rel_diff < convergence_thresh) and (niter > gate):   # em.rs:212
        return niter, True, True                             # em.rs:213 break
    niter = (niter + 1) & U32                                # em.rs:218
    return niter, not (niter < max_iter), False              # em.rs:181 while niter < max_iter


def test_rule_at_every_edge(shim):
    out = (C.c_uint32 * 4)()
    n_cells = 0
    for thresh, gate, max_iter in itertools.product((1e-3, 0.0, -1.0), (1, 50, U32), (1, 2, 52, 1000, U32)):
        rels = sorted({0.0, float(np.nextafter(thresh, -np.inf)), thresh, float(np.nextafter(thresh, np.inf)), 1.0})
        niters = sorted({n for n in (0, gate - 1, gate, gate + 1, max_iter - 2, max_iter - 1) if 0 <= n <= U32})
        for rel, niter, hist_cap in itertools.product(rels, niters, (0, 1, max_iter)):
            shim.shim_stopping_rule(niter, rel, max_iter, gate, hist_cap, thresh, C.byref(out))
            want = reference_step(niter, rel, thresh, gate, max_iter)
            # the record: iteration `niter`, as the rule sees it (before em.rs:218), at history[niter] while it fits
            want_hist = niter < hist_cap
            cell = f"thresh={thresh!r} rel={rel!r} gate={gate} niter={niter} max_iter={max_iter} hist_cap={hist_cap}"
            assert (out[0], bool(out[1]), bool(out[2])) == want, cell
            assert bool(out[3]) == want_hist, cell
            n_cells += 1
    assert n_cells > 2500   # (the grid did not collapse: 45 parameter sets x their distinct rel, niter and capacity values)


def test_rel_diff_term_signed_and_guarded(shim):
    thresh = 1e-5   # constants.rs MIN_READ_THRESH; em.rs:195 compares with `>`
    above = float(np.nextafter(thresh, np.inf))
    for prev in (thresh, above):
        for curr in (float(np.nextafter(prev, -np.inf)), 0.5 * prev, prev, float(np.nextafter(prev, np.inf)), 3.0 * prev):
            for rel in (0.0, -np.inf, 0.25):   # the loop's start value, a start that lets the sign show, a running maximum
                got = shim.shim_rel_diff_term(rel, prev, curr)
                if prev > thresh:
                    rd = (curr - prev) / prev                     # em.rs:198, signed
                    want = max(rel, rd)                           # em.rs:199
                    if rel == -np.inf:
                        assert got == rd and (np.sign(got) == np.sign(curr - prev))
                else:
                    want = rel                                    # at and below the threshold: no update
                assert got == want, (prev, curr, rel)
