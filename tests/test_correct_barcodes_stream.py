"""CPU tests of the barcode rule in a session (oarfish_amd/csrc/oem_barcode_correct.h, "The rule in a session";
oem_cells_stream_set_whitelist): the streamed host walk correct_barcodes_stream_host, through the testing library's hook
oem_test_correct_barcodes_stream_host, equals the one-shot walk correct_barcodes_host on the concatenation -- on every
case of tests/test_correct_barcodes.py and its random seeds, for multi 0 and 1, cut at every single position (the
hand-built cases: at every pair of positions) -- and on the mapped records' arrays where the input holds unmapped records;
the same comparison inside a stand-alone program under the address and undefined-behaviour sanitizers.
The new entry points are declared, exported by both libraries, bound and named in INTEGRATION.md, and refuse their
argument errors before any device use.  tests/test_cells_whitelist_stream_gpu.py holds the device session to the one call."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from oarfish_amd import _lib
from oarfish_amd import build as _b
from tests.test_correct_barcodes import (AMBIGUOUS, CORRECTED, EXACT, MISSING, NO_ID, NO_NEIGHBOUR, RANDOM_SEEDS, all_cases, hand_cases, host_walk,
                                         make_rule, pack, random_case, restate_rule)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "correct_barcodes_stream_main.cpp")
EXE = os.path.join(ROOT, "tests", "native", "correct_barcodes_stream_main")
HDRS = [os.path.join(ROOT, "oarfish_amd", "csrc", h) for h in ("oem_barcode_correct.h", "oem_barcode_table.h")]
HOOK = "oem_test_correct_barcodes_stream_host"
NEW = ["oem_cells_stream_set_whitelist", "oem_cells_stream_whitelist_copy"]
NO_PART = 0xFF


class Walker:
    """The hook on one case under one multi, its arrays packed once: walker(cuts, unmapped) runs the case's barcodes cut at
    `cuts` (ascending record positions) and returns (id, status, order, cell_rec_off, counts, cell_label, cell_corrected,
    rejected, deferred) as lists."""

    def __init__(self, case, multi):
        self.L = _lib.testing_lib()
        self.rule, self.keep = make_rule(case, multi)
        self.n, self.W = len(case["barcodes"]), len(case["whitelist"])
        self.blob, self.off = pack(case["barcodes"])
        if not len(self.blob):
            self.blob = np.zeros(1, dtype=np.uint8)

    def __call__(self, cuts, unmapped=None):
        n, W = self.n, self.W
        batch_off = np.array([0, *cuts, n], dtype=np.uint64)
        um = None if unmapped is None else np.ascontiguousarray(unmapped, dtype=np.uint8)
        ids = np.full(max(n, 1), 0xEEEEEEEE, dtype=np.uint32)
        status = np.full(max(n, 1), 0xEE, dtype=np.uint8)
        order = np.full(max(n, 1), 2 ** 64 - 1, dtype=np.uint64)
        cro = np.full(n + 1, 2 ** 64 - 1, dtype=np.uint64)
        label = np.full(W, 0xEEEEEEEE, dtype=np.uint32)
        corrected = np.full(W, 2 ** 64 - 1, dtype=np.uint64)
        counts = np.full(5, 2 ** 64 - 1, dtype=np.uint64)
        info = np.full(2, 2 ** 64 - 1, dtype=np.uint64)
        n_cells, n_acc = C.c_uint64(77), C.c_uint64(77)
        rc = self.L.oem_test_correct_barcodes_stream_host(
            C.addressof(self.rule), self.blob.ctypes.data if n else None, self.off.ctypes.data, batch_off.ctypes.data, len(batch_off) - 1,
            None if um is None else um.ctypes.data, ids.ctypes.data, status.ctypes.data, order.ctypes.data, cro.ctypes.data, label.ctypes.data,
            corrected.ctypes.data, C.byref(n_cells), C.byref(n_acc), counts.ctypes.data, info.ctypes.data)
        assert rc == _lib.OEM_OK, self.L.oem_last_error()
        nc, na = int(n_cells.value), int(n_acc.value)
        return (ids[:n].tolist(), status[:n].tolist(), order[:na].tolist(), cro[:nc + 1].tolist(), counts.tolist(), label[:nc].tolist(),
                corrected[:nc].tolist(), int(info[0]), int(info[1]))


def stream_walk(case, multi, cuts, unmapped=None):
    return Walker(case, multi)(cuts, unmapped)


def expect(one_shot, S=None, n=None):
    """What the streamed walk must give, from the one-shot walk's (id, status, order, cell_rec_off, counts) on the records S
    of an input of n records (S None: all of them): the same, indexed by the record's place in the whole input."""
    ids, status, order, cro, counts = one_shot
    if S is None:
        S, n = list(range(len(ids))), len(ids)
    full_id, full_st = [NO_ID] * n, [NO_PART] * n
    for k, i in enumerate(S):
        full_id[i], full_st[i] = ids[k], status[k]
    label = [ids[order[cro[c]]] for c in range(len(cro) - 1)]
    corrected = [sum(status[order[k]] == CORRECTED for k in range(cro[c], cro[c + 1])) for c in range(len(cro) - 1)]
    rejected = counts[NO_NEIGHBOUR] + counts[AMBIGUOUS] + counts[MISSING]
    return full_id, full_st, [S[k] for k in order], cro, counts, label, corrected, rejected


def cuttings(n, pairs):
    yield ()
    for a in range(n + 1):
        yield (a,)
    if pairs:
        yield from itertools.combinations_with_replacement(range(n + 1), 2)


def deferred_want(case, multi):
    """The records that wait for finish: under multi, the misses with two neighbours or more -- whatever the cutting."""
    if not multi:
        return 0
    wl, alphabet = case["whitelist"], case.get("alphabet", b"ACGT")
    known, out = set(wl), 0
    for b in case["barcodes"]:
        if b and b not in known:
            out += sum(1 for lab in wl if len(lab) == len(b) and sum(x != y for x, y in zip(lab, b)) == 1
                       and [y for x, y in zip(b, lab) if x != y][0] in alphabet) >= 2
    return out


# The hand-built stream of the GPU test (tests/test_cells_whitelist_stream_gpu.py builds its records around these
# barcodes): see STREAM's comments for what each record is there for.
WL5 = [b"AAAAAAAAAAAA", b"AATTAAAAAAAA", b"AATTCCAAAAAA", b"CCCCCCCCCCCC", b"CCGGCCCCCCCC"]
A0, A1, A2, C0, C1 = WL5
AB = b"AATAAAAAAAAA"       # between A0 and A1
BC = b"AATTCAAAAAAA"       # between A1 and A2
CD = b"CCGCCCCCCCCC"       # between C0 and C1
STREAM = [
    # barcode, unmapped
    (A2, 0),               # 0
    (AB, 0),               # 1  A0 and A1 tie at 0 when it arrives; A0 wins at the end: deferred, then corrected; the FIRST record of A0's cell
    (A1, 1),               # 2  unmapped and exact: counting it would make A0 / A1 tie at the end (and A1 beat A2 for record 14)
    (A0, 0),               # 3
    (CD, 0),               # 4  C0 and C1 tie at 0; C1 leads after 6, C0 after 9 and 10: the lead changes hands.  The first record of C0's cell
    (A2[:-1] + b"N", 0),   # 5  an N: corrected in its batch
    (C1, 0),               # 6
    (b"", 0),              # 7  missing
    (A0 + b"A", 0),        # 8  a length no label has
    (C0, 0),               # 9
    (C0, 0),               # 10
    (b"TTAAAAAAAAAA", 0),  # 11 a double error: no neighbour
    (A1, 0),               # 12
    (A0, 0),               # 13 -> n(A0) = 2 > n(A1) = 1
    (BC, 0),               # 14 A1 and A2 tie at 1 when it arrives and at the end: deferred, then rejected
    (CD, 0),               # 15
    (b"NNAAAAAAAAAA", 0),  # 16 two Ns: no neighbour
    (C0, 1),               # 17
    (AB, 0),               # 18
]
STREAM_CASE = dict(whitelist=WL5, barcodes=[b for b, _ in STREAM])
STREAM_UNMAPPED = [u for _, u in STREAM]


def test_the_streamed_walk_equals_the_one_shot_walk_at_every_cutting_of_the_hand_cases():
    for label, case, multi in all_cases():
        want = expect(host_walk(case, multi))
        n_def = deferred_want(case, multi)
        walker = Walker(case, multi)
        for cuts in cuttings(len(case["barcodes"]), pairs=True):
            got = walker(cuts)
            assert got[:8] == want, (label, cuts)
            assert got[8] == n_def, (label, cuts)


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
@pytest.mark.parametrize("multi", (0, 1))
def test_the_streamed_walk_on_random_cases_at_every_single_cut(seed, multi):
    case = random_case(seed)
    n = len(case["barcodes"])
    want = expect(host_walk(case, multi))
    n_def = deferred_want(case, multi)
    assert (n_def > 50) == bool(multi)
    walker = Walker(case, multi)
    for cuts in cuttings(n, pairs=False):
        got = walker(cuts)
        assert got[:8] == want and got[8] == n_def, cuts
    rng = np.random.default_rng(seed)
    cuts = tuple(sorted(int(x) for x in rng.integers(0, n + 1, size=40)))   # many batches, empty ones among them
    got = walker(cuts)
    assert got[:8] == want and got[8] == n_def


def test_the_hand_built_stream_holds_what_it_is_there_for():
    bcs, um = STREAM_CASE["barcodes"], STREAM_UNMAPPED
    S = [i for i in range(len(bcs)) if not um[i]]
    sub = dict(whitelist=WL5, barcodes=[bcs[i] for i in S])
    (ids, status, order, cro, counts), stats = restate_rule(sub, 1)
    at = {i: k for k, i in enumerate(S)}
    # deferred, then corrected: A0 wins 2 : 1 among the mapped records ...
    assert status[at[1]] == CORRECTED and ids[at[1]] == 0 and status[at[18]] == CORRECTED
    # ... and would tie 2 : 2 if the unmapped exact record 2 were counted
    all_ids, all_status = restate_rule(STREAM_CASE, 1)[0][:2]
    assert all_status[1] == AMBIGUOUS and all_status[18] == AMBIGUOUS
    # the lead changes hands: after record 6 C1 leads, at the end C0 does
    assert bcs[6] == C1 and bcs[9] == bcs[10] == C0 and status[at[4]] == CORRECTED and ids[at[4]] == 3
    # still tied at the end: deferred, then rejected (and corrected to A1 if the unmapped record 2 were counted)
    assert status[at[14]] == AMBIGUOUS and all_status[14] == CORRECTED and all_ids[14] == 1
    # a label whose first accepted record is a deferred one: A0's cell is opened by record 1, before record 3
    assert order[cro[1]] == at[1] and ids[order[cro[1]]] == 0 and [ids[order[cro[c]]] for c in range(len(cro) - 1)] == [2, 0, 3, 4, 1]
    assert order[cro[2]] == at[4]
    assert status[at[5]] == CORRECTED and status[at[7]] == MISSING and status[at[8]] == NO_NEIGHBOUR
    assert status[at[11]] == status[at[16]] == NO_NEIGHBOUR
    # under multi 0 every record between two labels is ambiguous in its batch
    st0 = restate_rule(sub, 0)[0][1]
    assert [st0[at[i]] for i in (1, 4, 14, 15, 18)] == [AMBIGUOUS] * 5


@pytest.mark.parametrize("multi", (0, 1))
def test_the_hand_built_stream_with_unmapped_records_at_every_pair_of_cuts(multi):
    bcs, um = STREAM_CASE["barcodes"], STREAM_UNMAPPED
    n = len(bcs)
    S = [i for i in range(n) if not um[i]]
    sub = dict(whitelist=WL5, barcodes=[bcs[i] for i in S])
    want = expect(host_walk(sub, multi), S, n)
    assert host_walk(sub, multi) == restate_rule(sub, multi)[0]
    walker = Walker(STREAM_CASE, multi)
    for cuts in cuttings(n, pairs=True):
        got = walker(cuts, STREAM_UNMAPPED)
        assert got[:8] == want, cuts
        assert got[8] == (5 if multi else 0)


def test_a_tie_that_lasts_is_deferred_then_rejected_and_an_unmapped_barcode_is_never_examined():
    case = dict(whitelist=WL5, barcodes=[A0, A1, AB, b"AA\x00A", CD])
    um = [0, 0, 0, 1, 0]
    got = stream_walk(case, 1, (2, 3), um)
    assert got[1] == [EXACT, EXACT, AMBIGUOUS, NO_PART, AMBIGUOUS] and got[7:] == (2, 2) and got[4] == [2, 0, 0, 2, 0]
    # the same 0 byte in a mapped record is the walk's error, by its index in the whole input
    L = _lib.testing_lib()
    rule, keep = make_rule(case, 1)
    blob, off = pack(case["barcodes"])
    batch_off = np.array([0, 2, 5], dtype=np.uint64)
    nc, na, info = C.c_uint64(0), C.c_uint64(0), np.zeros(2, dtype=np.uint64)
    rc = L.oem_test_correct_barcodes_stream_host(C.addressof(rule), blob.ctypes.data, off.ctypes.data, batch_off.ctypes.data, 2, None, None, None,
                                                 None, None, None, None, C.byref(nc), C.byref(na), None, info.ctypes.data)
    assert rc == _lib.OEM_ERR_ARG and b"the barcode of record 3 contains a 0 byte" in L.oem_last_error()
    del keep


# ---- the two walks in a stand-alone program under the address and undefined-behaviour sanitizers --------------------------
@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", os.path.join(ROOT, "include"), "-o", EXE, SRC])
    return EXE


def _case_text(case, multi, unmapped, pairs, hash_bits=64, slots0=8192):
    hexed = lambda b: b.hex() if b else "-"   # noqa: E731
    rows = [f"S {len(case['whitelist'])} {len(case['barcodes'])} {multi} {int(pairs)} {hash_bits} {slots0}"]
    rows += [hexed(w) for w in case["whitelist"]]
    rows += [f"{hexed(b)} {int(u)}" for b, u in zip(case["barcodes"], unmapped)]
    return "\n".join(rows) + "\n"


def test_the_streamed_walk_under_sanitizers(exe):
    """The program compares the two walks itself, at every cutting; here: its answers, and the sanitizers' silence.  Short
    hashes and a first capacity of 2 make every probe long and wrap, as tests/test_correct_barcodes.py's runs do."""
    n = len(STREAM_CASE["barcodes"])
    S = [i for i in range(n) if not STREAM_UNMAPPED[i]]
    text, want = "", []
    for multi in (0, 1):
        for bits, slots0 in ((64, 8192), (2, 2)):
            text += _case_text(STREAM_CASE, multi, STREAM_UNMAPPED, True, bits, slots0)
            _, status, order, cro, counts = restate_rule(dict(whitelist=WL5, barcodes=[STREAM_CASE["barcodes"][i] for i in S]), multi)[0]
            want.append(f"ok {(n + 1) * (n + 2) // 2} {len(order)} {len(cro) - 1} {counts[NO_NEIGHBOUR] + counts[AMBIGUOUS] + counts[MISSING]} "
                        f"{5 if multi else 0}")
    case = random_case(RANDOM_SEEDS[0], n_labels=240, n_records=400)
    rng = np.random.default_rng(7)
    um = (rng.random(400) < 0.1).astype(int).tolist()
    text += _case_text(case, 1, um, False)
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    rows = out.stdout.split("\n")[:-1]
    assert rows[:4] == want and rows[4].startswith("ok 401 ") and int(rows[4].split()[-1]) > 5, rows


def test_declared_exported_by_both_libraries_bound_and_documented():
    src = open(os.path.join(ROOT, "include", "oarfish_em.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+oem_cells_stream_set_whitelist\s*\(\s*oem_cells_stream \*s,\s*const oem_barcode_rule \*rule\s*\)\s*;", code)
    m = re.search(r"\bint\s+oem_cells_stream_whitelist_copy\s*\(([^;]*)\)\s*;", code)
    assert m and [a.strip() for a in m.group(1).split(",")] == ["const oem_cells_stream *s", "uint32_t *out_cell_wl_id",
                                                                "uint64_t *out_cell_bc_corrected", "uint64_t *out_counts"]
    assert re.search(r"#define OEM_CELLS_STREAM_INFO_BARCODE_REJECTED\s+13u", src) and _lib.OEM_CELLS_STREAM_INFO_BARCODE_REJECTED == 13
    assert re.search(r"#define OEM_CELLS_STREAM_INFO_BARCODE_DEFERRED\s+14u", src) and _lib.OEM_CELLS_STREAM_INFO_BARCODE_DEFERRED == 14
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        for path in (_b.LIB_PATH, _b.TESTING_LIB_PATH):
            out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
            assert name in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, path
        assert name in _lib.ABI_SYMBOLS and "`%s`" % name in doc
    assert HOOK in _b.TESTING_HOOKS and len(getattr(_lib.testing_lib(), HOOK).argtypes) == 16
    assert not hasattr(_lib.lib(), HOOK)
    # the open end is closed where it was stated
    assert "do not take the rule yet" not in src
    assert "do not take a whitelist yet" not in open(os.path.join(ROOT, "README.md")).read()
    hdr = open(os.path.join(ROOT, "oarfish_amd", "csrc", "oem_barcode_correct.h")).read()
    assert "THE RULE IN A SESSION" in hdr and "correct_barcodes_stream_host" in hdr and "the sessions differ" in hdr


def test_null_sessions_and_python_argument_errors_before_any_device_use():
    import oarfish_amd
    from oarfish_amd.single_cell import SingleCellArgs
    L = _lib.lib()
    assert L.oem_cells_stream_set_whitelist(None, None) == _lib.OEM_ERR_ARG and b"NULL session" in L.oem_last_error()
    assert L.oem_cells_stream_whitelist_copy(None, None, None, None) == _lib.OEM_ERR_ARG and b"oem_cells_stream_whitelist_copy" in L.oem_last_error()
    tl = np.full(4, 1000, dtype=np.uint64)
    F = dict()
    with pytest.raises(ValueError, match="whitelist goes with barcodes"):
        oarfish_amd.CellsStream(4, filters=F, txp_len=tl, whitelist=WL5)
    with pytest.raises(ValueError, match="collated=False"):
        oarfish_amd.CellsStream(4, filters=F, txp_len=tl, barcodes=True, whitelist=WL5)
    with pytest.raises(ValueError, match="barcode_multi goes with whitelist"):
        oarfish_amd.CellsStream(4, filters=F, txp_len=tl, barcodes=True, collated=False, barcode_multi=True)
    with pytest.raises(ValueError, match="collated=False"):
        SingleCellArgs("out", whitelist=WL5, collated=True)
    with pytest.raises(ValueError, match="barcode_multi goes with whitelist"):
        SingleCellArgs("out", barcode_multi=True)
