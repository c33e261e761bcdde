"""CPU tests of the projected filter (genome mode): the pure headers oem_filter_projected.h and oem_exp_f32.h in a
stand-alone program under the address and undefined-behaviour sanitizers, held to tests/projected_ref.py
(AlignmentFilters::filter_projected, oarfish_types.rs:1179-1297) and to libm's expf; oem_builder_add_projected_groups
against the oem_builder_add_projected_group loop and the restatement; the generator of synthetic projected records."""
import os
import struct
import subprocess

import numpy as np
import pytest

from oarfish_amd import _lib, synth
from oarfish_amd.builder import PROJ_RECORD, StoreBuilder
from oracle import filter_py as fp

from tests import projected_ref as pr
from tests.filter_common import f32_bits, filters_dict, state
from tests.filter_common import pack as pack_plain, random_groups as random_plain_groups

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "filter_projected_main.cpp")
EXE = os.path.join(HERE, "native", "filter_projected_main")
HDRS = [os.path.join(ROOT, "oarfish_amd", "csrc", h) for h in ("oem_filter_projected.h", "oem_filter.h", "oem_exp_f32.h")]
DISCARD = [n for n, _ in _lib.DiscardTableC._fields_]
CODE = {"similarity": 0, "score": 1, "combined": 2}


# ---------------------------------------------------------------------------------------------------------------------
# the headers, stand-alone, under sanitizers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                               "-o", EXE, SRC])
    return EXE


def run(exe, text, n_answers):
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[-1] == "" and len(out) == n_answers + 1
    return out[:-1]


def f64_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def head_lines(F, txp_len, beta, source):
    return (f"F {F.five_prime_clip} {F.three_prime_clip} {f32_bits(F.score_threshold):x} {f32_bits(F.min_aligned_fraction):x} "
            f"{F.min_aligned_len} {F.which_strand} {f32_bits(F.score_prob_denom):x}\n"
            f"O {f32_bits(beta):x} {CODE[source]}\n"
            f"T {len(txp_len)} " + " ".join(str(int(v)) for v in txp_len) + "\n")


def group_lines(g, read_len):
    return f"G {len(g)} {read_len}\n" + "".join(
        f"{x.ref_id} {x.start} {x.end} {x.aligned_len} {x.query_aligned_len} {x.aln_score} {2 if x.reverse else 0} "
        f"{f64_bits(x.similarity):x}\n" for x in g)


def check_against_restatement(exe, F, txp_len, groups, read_lens, beta, source):
    """verdicts, counters, emitted coordinates and the bit pattern of f, group by group"""
    text = head_lines(F, txp_len, beta, source) + "".join(group_lines(g, rl) for g, rl in zip(groups, read_lens))
    out = run(exe, text, 3 + len(groups))[3:]
    answers = []
    for g, rl, line in zip(groups, read_lens, out):
        head, counts, emitted = line.split("|")
        verdict, n_kept, _best_sim, _best_score, flags, _bad = (int(v, 16) if k == 2 else int(v) for k, v in enumerate(head.split()))
        dt = fp.Store().dt
        want = pr.filter_projected(dt, F, txp_len, g, rl, beta, source) if g else []
        assert n_kept == len(want) and not (flags & 1), (g, line)
        assert dict(zip(DISCARD, (int(v) for v in counts.split()))) == dt, (g, line)
        assert verdict == (2 if dt["valid_best_aln"] else 1 if dt["discard_aln_frac"] else 0)
        got = [t.split(":") for t in emitted.split()]
        assert len(got) == len(want)
        for (i, s, e, fb), (ref_id, ws, we, _strand, wf) in zip(got, want):
            assert g[int(i)].ref_id == ref_id and (int(s), int(e)) == (ws, we), (g, line)
            assert int(fb, 16) == f32_bits(wf), (g, i, fb, wf)
        answers.append((verdict, n_kept, [(int(i), int(s), int(e), np.uint32(int(fb, 16)).view(np.float32)) for i, s, e, fb in got], dt))
    return answers


@pytest.mark.parametrize("source", pr.SOURCES)
def test_projected_header_against_the_restatement_on_the_edge_list(exe, source):
    seen = {}
    for name, F, txp_len, g, rl in pr.edge_groups():
        seen[name] = check_against_restatement(exe, F, txp_len, [g], [rl], 10.0, source)[0]
    only = lambda name, counter: seen[name][3][counter] == 1 and sum(seen[name][3].values()) - seen[name][3]["valid_best_aln"] == 1  # noqa: E731
    # hand-checked: the verdicts 0 no counter moves, 1 aligned fraction, 2 valid
    assert seen["empty"][:2] == (0, 0) and seen["one"][:2] == (2, 1)
    assert only("ori forward only", "discard_ori") and only("ori reverse only", "discard_ori") and only("aln_len", "discard_aln_len")
    assert only("3p", "discard_3p") and only("5p", "discard_5p") and only("score", "discard_score") and only("aln_frac", "discard_aln_frac")
    assert [k[0] for k in seen["score"][2]] == [0, 2]                            # 0.9499 / 1.0 < 0.95 <= 0.9501 / 1.0
    assert seen["tie: the first decides the fraction"][:2] == (1, 0)            # 700 / 1500 < 0.5 although the second covers it
    assert seen["tie: the first decides the fraction (kept)"][:2] == (2, 2)
    for name in ("best similarity 0", "best similarity negative", "nan only"):   # no counter moves
        assert seen[name][:2] == (0, 0) and sum(seen[name][3].values()) == 0
    assert [k[0] for k in seen["nan similarity"][2]] == [1] and seen["nan similarity"][3]["discard_score"] == 2
    assert seen["read_len 0"][:2] == (1, 0) and seen["read_len 0, fraction 0 allowed"][:2] == (2, 1)
    assert seen["threshold 1.5"][:2] == (2, 0) and seen["threshold 1.5"][3]["valid_best_aln"] == 1   # valid, no row
    assert [k[1:3] for k in seen["start 0 and end beyond the transcript"][2]] == [(1, 2000), (2000, 2000)]   # the clamps
    apart = [k[3] for k in seen["best score and best similarity apart"][2]]      # best similarity 0.9 (record 0), best score 80 (record 1)
    want = {"similarity": [0.0, np.float32(0.7 - 0.9) * np.float32(10.0), np.float32(0.8 - 0.9) * np.float32(10.0)],
            "score": [-6.0, 0.0, -12.0]}
    if source in want:
        assert [float(v) for v in apart] == [float(np.float32(v)) for v in want[source]]
    else:
        assert apart[0] == np.float32(-6.0) and apart[1] == np.float32(0.0) + np.float32(10.0) * np.float32(0.7 - 0.9)
    wraps = [k[3] for k in seen["score difference wraps"][2]]
    if source == "score":                                                        # -2^31 - (2^31 - 1) wraps to +1
        assert [float(v) for v in wraps] == [0.0, float(np.float32(1.0) / np.float32(5.0))]
    assert seen["300 records"][1] > 100


@pytest.mark.parametrize("seed", [21, 22])
def test_projected_header_against_the_restatement_on_random_groups(exe, seed):
    F, txp_len, groups, read_lens = pr.random_groups(seed, 400)
    n_rows = 0
    for source in pr.SOURCES:
        got = check_against_restatement(exe, F, txp_len, groups, read_lens, 10.0 if source != "combined" else 3.5, source)
        n_rows = sum(1 for a in got if a[1])
    assert n_rows > 40


def test_projected_header_flags_argument_errors_and_big_scores(exe):
    F = fp.Filters(which_strand=1)
    ok = lambda t, sc=0, **kw: pr.PRec(t, 10, 1500, 1400, 1400, 0.9, sc, **kw)      # noqa: E731
    gs = [[ok(0), ok(2)],                                 # ref_id 2 >= 2: record 1
          [ok(0), ok(0), ok(1, reverse=True)],            # transcript 1 has length 0: record 2, although the strand test drops it
          [ok(0, 2 ** 24 + 1)], [ok(0, 2 ** 24)], [ok(0, -2 ** 24 - 1, reverse=True)], [ok(0, -2 ** 24)]]
    text = head_lines(F, [2000, 0], 10.0, "score") + "".join(group_lines(g, 1500) for g in gs)
    heads = [[int(v, 16) if k == 2 else int(v) for k, v in enumerate(ln.split("|")[0].split())] for ln in run(exe, text, 3 + len(gs))[3:]]
    assert heads[0][4:] == [1, 1] and heads[1][4:] == [1, 2]
    assert [h[4] for h in heads[2:]] == [2, 0, 2, 0]


def test_exp_candidate_is_libm_expf_wherever_it_is_sure(exe):
    lo, hi = f32_bits(-0.0), f32_bits(-104.0)             # the negative f32 in bit order: -0 .. -104
    n, n_unsure, n_sure_bad, n_cand_bad = (int(v) for v in run(exe, f"S {lo:x} {hi:x} 991\n", 1)[0].split())
    assert n == (hi - lo) // 991 + 1 > 1_000_000
    assert n_sure_bad == 0                                # no sure candidate differs from libm's expf
    assert n_unsure <= 0.01 * n                           # a cap, not a measurement
    assert n_cand_bad <= n_unsure
    # the domain's ends and what lies outside it
    one = lambda x: [int(v, 16) for v in run(exe, f"X {f32_bits(x):x}\n", 1)[0].split()]      # noqa: E731
    assert one(0.0) == [f32_bits(1.0), 1, f32_bits(1.0)] and one(-0.0) == [f32_bits(1.0), 1, f32_bits(1.0)]
    for x in (1e-30, 0.5, 88.0, 1000.0, float("inf"), float("-inf"), float("nan"), -88.0, -100.0, -104.0, -1000.0):
        assert one(x)[1] == 0, x                          # positive, not finite, or a result below FLT_MIN: libm is asked
    c, sure, want = one(-87.0)
    assert sure == 0 or c == want


# ---------------------------------------------------------------------------------------------------------------------
# host batch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", pr.SOURCES)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_projected_batch_equals_the_loop_and_the_restatement(seed, source):
    F, txp_len, groups, read_lens = pr.random_groups(seed, 500)
    groups[5], groups[-1] = [], []                                    # empty groups: nothing is touched (:703-705)
    beta = [10.0, 4.0, 25.0][seed - 1]
    rec, off, rl = pr.pack(groups, read_lens)
    want, want_kept = pr.host_loop(F, txp_len, groups, read_lens, beta, source)
    ref, ref_kept = pr.oracle_loop(F, txp_len, groups, read_lens, beta, source)
    b = StoreBuilder(filters_dict(F), txp_len)
    kept = b.add_projected_groups(rec, off, rl, beta=beta, prob_source=source)
    assert np.array_equal(kept, want_kept) and np.array_equal(kept, ref_kept)
    assert state(b) == state(want) == pr.oracle_state(ref)            # every array bit for bit, the dims, the discard table
    R = b.dims()[0]
    assert R > 40 and np.flatnonzero(kept)[R - 1] >= R - 1            # row r is the r-th group with kept > 0
    dt = b.discard_table()
    assert dt["no_mapping"] == dt["no_valid_aln"] == dt["discard_supp"] == 0
    # appending to a non-empty builder; a batch without groups changes nothing
    before = state(b)
    assert len(b.add_projected_groups(np.zeros(0, dtype=PROJ_RECORD), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint64))) == 0
    assert state(b) == before
    b.add_projected_groups(rec, off, rl, beta=beta, prob_source=source)
    pr.oracle_loop(F, txp_len, groups, read_lens, beta, source, into=ref)
    assert state(b) == pr.oracle_state(ref)


def test_projected_and_plain_batches_in_turn():
    F, txp_len, groups, read_lens = pr.random_groups(7, 300)
    _, _, plain = random_plain_groups(7, 300, T=len(txp_len))       # (its records only: the builder has one set of filters)
    ref = fp.Store()
    b = StoreBuilder(filters_dict(F), txp_len)
    for lo in (0, 100, 200):
        b.add_projected_groups(*pr.pack(groups[lo:lo + 100], read_lens[lo:lo + 100]), beta=10.0, prob_source="combined")
        pr.oracle_loop(F, txp_len, groups[lo:lo + 100], read_lens[lo:lo + 100], 10.0, "combined", into=ref)
        b.add_groups(*pack_plain(plain[lo:lo + 100]))
        for g in plain[lo:lo + 100]:
            fp.add_group(ref, F, txp_len, g)
    assert state(b) == pr.oracle_state(ref) and b.dims()[0] > 60
    assert b.discard_table()["no_valid_aln"] + b.discard_table()["no_mapping"] > 0    # (the plain batches' own counters)


def test_projected_batch_is_atomic_and_checks_its_arguments():
    F, txp_len, groups, read_lens = pr.random_groups(11, 200)
    txp_len = np.array(txp_len)
    groups.append([pr.PRec(3, 10, 900, 800, 800, 0.9), pr.PRec(len(txp_len), 10, 900, 800, 800, 0.9)])
    read_lens.append(900)
    rec, off, rl = pr.pack(groups, read_lens)
    b = StoreBuilder(filters_dict(F), txp_len)
    b.add_projected_groups(*pr.pack(groups[:50], read_lens[:50]))
    before = state(b)
    with pytest.raises(_lib.OemError) as ei:
        b.add_projected_groups(rec, off, rl)
    assert ei.value.code == _lib.OEM_ERR_ARG and f"record {len(rec) - 1}:" in str(ei.value) and "n_txps" in str(ei.value)
    assert state(b) == before                                         # the 200 good groups before it left no trace
    with pytest.raises(_lib.OemError) as ei:
        b.add_projected_group(rec[-2:], 900)
    assert ei.value.code == _lib.OEM_ERR_ARG and state(b) == before
    zero = txp_len.copy(); zero[3] = 0                                # a transcript of length 0
    with StoreBuilder(filters_dict(F), zero) as bz:
        with pytest.raises(_lib.OemError) as ei:
            bz.add_projected_groups(rec[:-1], np.concatenate([off[:-1], [len(rec) - 1]]).astype(np.uint64), rl)
        first = int(np.flatnonzero(rec["ref_id"] == 3)[0])          # the first record that names it, whatever becomes of it
        assert ei.value.code == _lib.OEM_ERR_ARG and f"record {first}:" in str(ei.value) and "length 0" in str(ei.value)
        assert bz.dims() == (0, 0) and sum(bz.discard_table().values()) == 0
    L = _lib.lib()
    import ctypes as C
    po = _lib.ProjOptsC(10.0, 0)
    n = len(groups)
    args = lambda r, o, l, p: (b.handle, r, o, l, n, p, None)         # noqa: E731
    good = (rec.ctypes.data, off.ctypes.data, rl.ctypes.data, C.addressof(po))
    for k in range(4):
        a = list(good); a[k] = None
        assert L.oem_builder_add_projected_groups(*args(*a)) == _lib.OEM_ERR_ARG, k
    bad = off.copy(); bad[0] = 1
    assert L.oem_builder_add_projected_groups(*args(good[0], bad.ctypes.data, good[2], good[3])) == _lib.OEM_ERR_ARG
    bad = off.copy(); bad[7] = bad[8] + 1
    assert L.oem_builder_add_projected_groups(*args(good[0], bad.ctypes.data, good[2], good[3])) == _lib.OEM_ERR_ARG
    assert b"decreases" in L.oem_last_error()
    po3 = _lib.ProjOptsC(10.0, 3)
    assert L.oem_builder_add_projected_groups(*args(good[0], good[1], good[2], C.addressof(po3))) == _lib.OEM_ERR_ARG
    assert b"prob_source" in L.oem_last_error()
    with pytest.raises(ValueError):
        b.add_projected_groups(rec, off, rl, prob_source="best")
    with pytest.raises(ValueError):
        b.add_projected_groups(rec, off, rl[:-1])
    assert state(b) == before


def test_projected_device_forms_fail_loudly_without_a_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    import oarfish_amd
    F, txp_len, groups, read_lens = pr.random_groups(12, 20)
    rec, off, rl = pr.pack(groups, read_lens)
    b = StoreBuilder(filters_dict(F), txp_len)
    for source, beta in (("similarity", 10.0), ("score", 10.0), ("combined", float("inf"))):   # the last: a host-loop batch
        with pytest.raises(_lib.OemError) as ei:
            b.add_projected_groups(rec, off, rl, beta=beta, prob_source=source, device=0)
        assert ei.value.code == _lib.OEM_ERR_NO_DEVICE and b.dims() == (0, 0)
        with pytest.raises(_lib.OemError) as ei:
            oarfish_amd.DeviceStore.from_projected_records(filters_dict(F), txp_len, rec, off, rl, beta=beta, prob_source=source)
        assert ei.value.code == _lib.OEM_ERR_NO_DEVICE
    bad = off.copy(); bad[0] = 1                                      # argument errors come first
    with pytest.raises(_lib.OemError) as ei:
        b.add_projected_groups(rec, bad, rl, device=0)
    assert ei.value.code == _lib.OEM_ERR_ARG


def test_make_projected_records_gives_the_store_back():
    st = synth.make_store(3000, 200, seed=77)
    sr = synth.make_projected_records(st)
    b = StoreBuilder(sr.filters, sr.txp_len)
    kept = b.add_projected_groups(sr.records, sr.group_off, sr.read_len, beta=sr.beta)
    rp, tid, p, s, e, sd = b.export()
    assert np.array_equal(kept, sr.kept) and b.discard_table() == sr.discard
    assert np.array_equal(rp, st.row_ptr) and np.array_equal(tid, st.tid)
    # f = (float)(ln p / beta) * beta carries two f32 roundings of relative size 2^-24 each, exp turns them into
    # |f| * 2^-23, and libm's expf and the store's own rounding of p add an ulp: 2^-23 * (|ln p| + 2)
    assert np.all(np.abs(p.astype(np.float64) - st.as_prob) <= 2.0 ** -23 * (np.abs(np.log(st.as_prob.astype(np.float64))) + 2) * st.as_prob)
    reachable = ("discard_5p", "discard_3p", "discard_score", "discard_aln_frac", "discard_aln_len", "discard_ori", "valid_best_aln")
    assert all(sr.discard[k] > 0 for k in reachable) and all(v == 0 for k, v in sr.discard.items() if k not in reachable)
    assert len(sr.records) > st.nnz and (kept == 0).sum() > 50
    assert np.all(1 <= s) and np.all(s <= e) and np.all(e <= sr.txp_len[tid])
    with StoreBuilder(sr.filters, sr.txp_len) as b2:                  # the score source gives the same gaps back
        b2.add_projected_groups(sr.records, sr.group_off, sr.read_len, beta=sr.beta, prob_source="score")
        np.testing.assert_allclose(b2.export()[2], st.as_prob, rtol=2e-7)
        assert b2.discard_table() == sr.discard

