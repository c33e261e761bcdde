"""CPU tests of the batched filter: oem_builder_add_groups against the oem_builder_add_group loop and against
oracle/filter_py.add_group (AlignmentFilters::filter, oarfish_types.rs:955-1130), the pure header oem_filter.h in a
stand-alone program under the address and undefined-behaviour sanitizers, and the rule of the expf table the device
looks as_prob up in."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oarfish_amd import _lib
from oarfish_amd.builder import ALN_RECORD, StoreBuilder
from oracle import filter_py as fp

from tests.filter_common import edge_groups, f32_bits, libm_expf, filters_dict, host_loop, oracle_loop, pack, random_groups, state

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "filter_main.cpp")
EXE = os.path.join(HERE, "native", "filter_main")
HDR = os.path.join(ROOT, "oarfish_amd", "csrc", "oem_filter.h")
DISCARD = [n for n, _ in _lib.DiscardTableC._fields_]


# ---------------------------------------------------------------------------------------------------------------------
# host batch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_add_groups_equals_the_add_group_loop_and_the_oracle(seed):
    F, txp_len, groups = random_groups(seed, 800)
    groups[5] = []                                                    # empty groups: nothing is touched (:677)
    groups[-1] = []
    rec, off = pack(groups)
    want, want_kept = host_loop(F, txp_len, groups)
    ref, ref_kept = oracle_loop(F, txp_len, groups)
    b = StoreBuilder(filters_dict(F), txp_len)
    kept = b.add_groups(rec, off)
    assert np.array_equal(kept, want_kept) and np.array_equal(kept, ref_kept)
    assert state(b) == state(want)
    rp, tid, p, s, e, sd = b.export()
    assert list(rp) == ref.row_ptr and list(tid) == ref.tid and list(s) == ref.start and list(e) == ref.end
    assert list(sd) == ref.strand and b.discard_table() == ref.dt
    assert np.array_equal(p.view(np.uint32), np.asarray(ref.as_prob, dtype=np.float32).view(np.uint32))  # bit-exact f32
    assert len(rp) - 1 > 20 and np.flatnonzero(kept)[len(rp) - 2] >= len(rp) - 2   # row r is the r-th group with kept > 0
    # appending to a non-empty builder; a batch without groups changes nothing
    before = state(b)
    assert len(b.add_groups(np.zeros(0, dtype=ALN_RECORD), np.zeros(1, dtype=np.uint64))) == 0
    assert state(b) == before
    b.add_groups(rec, off)
    host_loop(F, txp_len, groups, into=want)
    assert state(b) == state(want)


def test_add_groups_is_atomic_and_checks_group_off():
    F, txp_len, groups = random_groups(11, 200)
    groups.append([fp.Rec(3, 10, 900, 800, 500, 900), fp.Rec(len(txp_len), 10, 900, 800, 500, 900)])
    rec, off = pack(groups)
    b = StoreBuilder(filters_dict(F), txp_len)
    b.add_groups(*pack(groups[:50]))
    before = state(b)
    with pytest.raises(_lib.OemError) as ei:
        b.add_groups(rec, off)
    assert ei.value.code == _lib.OEM_ERR_ARG and f"record {len(rec) - 1}:" in str(ei.value) and "n_txps" in str(ei.value)
    assert state(b) == before                                         # the 200 good groups before it left no trace
    L = _lib.lib()
    kept = np.zeros(len(groups), dtype=np.uint32)
    assert L.oem_builder_add_groups(b.handle, rec.ctypes.data, None, len(groups), kept.ctypes.data) == _lib.OEM_ERR_ARG
    bad = off.copy(); bad[0] = 1
    assert L.oem_builder_add_groups(b.handle, rec.ctypes.data, bad.ctypes.data, len(groups), None) == _lib.OEM_ERR_ARG
    bad = off.copy(); bad[7] = bad[8] + 1
    assert L.oem_builder_add_groups(b.handle, rec.ctypes.data, bad.ctypes.data, len(groups), None) == _lib.OEM_ERR_ARG
    assert b"decreases" in L.oem_last_error()
    assert L.oem_builder_add_groups(b.handle, None, off.ctypes.data, len(groups), None) == _lib.OEM_ERR_ARG
    assert L.oem_builder_add_groups(None, rec.ctypes.data, off.ctypes.data, len(groups), None) == _lib.OEM_ERR_ARG
    assert state(b) == before
    # an unmapped record's ref_id is never looked at
    ok = [[fp.Rec(2 ** 32 - 1, 0, 0, 0, None, 100, unmapped=True)]]
    assert list(b.add_groups(*pack(ok))) == [0]


def test_device_forms_fail_loudly_without_a_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    import oarfish_amd
    F, txp_len, groups = random_groups(12, 20)
    rec, off = pack(groups)
    b = StoreBuilder(filters_dict(F), txp_len)
    with pytest.raises(_lib.OemError) as ei:
        b.add_groups(rec, off, device=0)
    assert ei.value.code == _lib.OEM_ERR_NO_DEVICE and b.dims() == (0, 0)
    with pytest.raises(_lib.OemError) as ei:
        oarfish_amd.DeviceStore.from_records(filters_dict(F), txp_len, rec, off)
    assert ei.value.code == _lib.OEM_ERR_NO_DEVICE
    bad = off.copy(); bad[0] = 1                                      # argument errors come first
    with pytest.raises(_lib.OemError) as ei:
        b.add_groups(rec, bad, device=0)
    assert ei.value.code == _lib.OEM_ERR_ARG


def test_make_records_gives_the_store_back():
    from oarfish_amd import synth
    st = synth.make_store(3000, 200, seed=77)
    sr = synth.make_records(st)
    b = StoreBuilder(sr.filters, sr.txp_len)
    kept = b.add_groups(sr.records, sr.group_off)
    rp, tid, p, s, e, sd = b.export()
    assert np.array_equal(kept, sr.kept) and b.discard_table() == sr.discard
    assert np.array_equal(rp, st.row_ptr) and np.array_equal(tid, st.tid)
    np.testing.assert_allclose(p, st.as_prob, rtol=2e-7)             # the gaps are the store's (numpy's exp there, libm's here)
    assert all(v > 0 for v in sr.discard.values()) and len(sr.records) > st.nnz
    assert np.all(s <= e) and np.all(e <= sr.txp_len[tid])


# ---------------------------------------------------------------------------------------------------------------------
# oem_filter.h, stand-alone, under sanitizers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-o", EXE, SRC])
    return EXE


def run(exe, text, n_answers):
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[-1] == "" and len(out) == n_answers + 1
    return out[:-1]


def filters_line(F):
    return (f"F {F.five_prime_clip} {F.three_prime_clip} {f32_bits(F.score_threshold):x} {f32_bits(F.min_aligned_fraction):x} "
            f"{F.min_aligned_len} {F.which_strand} {f32_bits(F.score_prob_denom):x}\n")


def group_lines(g):
    rec, _ = pack([g])
    return f"G {len(g)}\n" + "".join(f"{r['ref_id']} {r['aln_start']} {r['aln_end']} {r['aln_span']} {r['score']} {r['seq_len']} {r['flags']}\n" for r in rec)


def check_against_oracle(exe, F, txp_len, groups):
    text = filters_line(F) + f"T {len(txp_len)} " + " ".join(str(int(v)) for v in txp_len) + "\n" + "".join(group_lines(g) for g in groups)
    out = run(exe, text, 2 + len(groups))[2:]
    answers = []
    for g, line in zip(groups, out):
        head, counts, emitted = line.split("|")
        verdict, n_kept, best, flags, _bad = (int(v) for v in head.split())
        ref = fp.Store()
        want = fp.add_group(ref, F, txp_len, g)
        assert n_kept == want and flags == 0, (g, line)
        assert dict(zip(DISCARD, (int(v) for v in counts.split()))) == ref.dt, (g, line)
        pairs = [tuple(int(v) for v in t.split(":")) for t in emitted.split()]
        assert len(pairs) == want
        # the table index reproduces the oracle's probability: expf((float)(-gap) / D) == its as_prob, bit for bit
        for (i, gap), p in zip(pairs, ref.as_prob):
            assert g[i].ref_id == ref.tid[pairs.index((i, gap))]
            got = fp._libm.expf(ctypes.c_float(float(np.float32(-gap) / np.float32(F.score_prob_denom))))
            assert np.float32(got).view(np.uint32) == np.float32(p).view(np.uint32), (g, i, gap)
        answers.append((verdict, n_kept, best, pairs))
    return answers


def test_filter_header_against_the_oracle_on_the_edge_list(exe):
    seen = {}
    for name, F, txp_len, g in edge_groups():
        seen[name] = check_against_oracle(exe, F, txp_len, [g])[0]
    # hand-checked: the verdicts 0 empty, 1 no mapping, 2 no valid alignment, 3 aligned fraction, 4 valid
    assert seen["empty"][:2] == (0, 0) and seen["unmapped only"][:2] == (1, 0) and seen["non-positive best"][:2] == (2, 0)
    assert seen["aln_frac"][:2] == (3, 0) and seen["one"] == (4, 1, 1000, [(0, 0)])
    assert seen["tie: the first decides the fraction"][:2] == (3, 0)          # 700 / 1500 < 0.5 although the second covers it
    assert seen["tie: the first decides the fraction (kept)"][3] == [(0, 0), (1, 0)]
    assert seen["score"][3] == [(0, 0), (2, 50)]                               # 949 / 1000 < 0.95 <= 950 / 1000
    assert seen["no score, threshold 0"][3] == [(0, 0), (1, 700)]              # kept with gap = best
    assert seen["no score, threshold -1"][3] == [(0, 0), (1, 700), (2, 1000)]
    assert seen["no score, default threshold"][3] == [(0, 0)]
    assert seen["seq_len on the third record"][3] == [(0, 0), (1, 10), (2, 20)]  # 1400 / 2000; without a length the fraction is 0
    assert seen["no seq_len at all"][:2] == (3, 0)                             # fraction 0
    assert seen["threshold 1.5"][:2] == (4, 0)                                 # valid_best_aln counted, no row
    assert seen["table end"][3] == [(0, 0), (1, 519), (2, 520), (3, 521), (4, 1100)]
    assert seen["score wraps as i32"][2] == 1000
    assert seen["300 records"][1] > 100


@pytest.mark.parametrize("seed", [21, 22])
def test_filter_header_against_the_oracle_on_random_groups(exe, seed):
    F, txp_len, groups = random_groups(seed, 400)
    got = check_against_oracle(exe, F, txp_len, groups)
    assert sum(1 for a in got if a[1]) > 20


def test_filter_header_flags_bad_ref_and_big_scores(exe):
    F = fp.Filters()
    text = filters_line(F) + "T 2 2000 2000\n"
    gs = [[fp.Rec(0, 10, 1500, 1400, 1000, 1500), fp.Rec(2, 10, 1500, 1400, 1000, None)],       # ref_id 2 >= 2: record 1
          [fp.Rec(0, 10, 1500, 1400, 2 ** 24 + 1, 1500)], [fp.Rec(0, 10, 1500, 1400, 2 ** 24, 1500)],
          [fp.Rec(0, 10, 1500, 1400, -2 ** 24 - 1, 1500, supp=True)],                              # a discarded record counts too
          [fp.Rec(5, 0, 0, 0, 2 ** 30, 100, unmapped=True)]]                                       # an unmapped one does not
    out = run(exe, text + "".join(group_lines(g) for g in gs), 2 + len(gs))[2:]
    heads = [[int(v) for v in ln.split("|")[0].split()] for ln in out]
    assert heads[0][3] == 1 and heads[0][4] == 1
    assert heads[1][3] == 2 and heads[2][3] == 0 and heads[3][3] == 2 and heads[4][3] == 0


# ---------------------------------------------------------------------------------------------------------------------
# the table rule
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [0.5, 2.5, 5.0, 10.0])
def test_table_rule(exe, D):
    out = run(exe, f"P {f32_bits(D):x}\n", 1)[0].split()
    n, tab = int(out[0]), np.array([int(v, 16) for v in out[1:]], dtype=np.uint32).view(np.float32)
    assert n == len(tab) and abs(n - (104 * D + 1)) <= 2
    for g in range(n):
        want = libm_expf(np.float32(-g) / np.float32(D))
        assert tab[g].view(np.uint32) == want.view(np.uint32), g
    assert tab[-1].view(np.uint32) == 0 and tab[-2] != 0 and tab[0] == 1.0   # ends at the first +0.0
    for k in range(1, 26):                                            # beyond the end libm gives +0.0 as well
        for g in (2 ** k - 1, 2 ** k, 2 ** k + 1):
            if g >= n:
                assert libm_expf(np.float32(-g) / np.float32(D)).view(np.uint32) == 0, g


def test_table_is_refused_where_the_host_loop_must_run(exe):
    for D in (0.0, -5.0, float("inf"), float("nan"), 1e30, 50000.0):
        assert run(exe, f"P {f32_bits(D):x}\n", 1)[0] == "0", D
    n = int(run(exe, f"P {f32_bits(1e-30):x}\n", 1)[0].split()[0])
    assert n == 2                                                     # 1, then 0 at once
