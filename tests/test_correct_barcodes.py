"""CPU tests of barcode correction against a whitelist -- oem_correct_barcodes, oem_em_run_cells_records_whitelist_sparse:
declared, exported by both libraries and bound; the host walk of the rule (oarfish_amd/csrc/oem_barcode_correct.h,
correct_barcodes_host) against a walk written here; the same walk in a stand-alone program under the address and
undefined-behaviour sanitizers; the argument errors before any device use; the Python wrappers' own checks; the synthetic
whitelist and barcode errors.

The walk here knows nothing of the C++ one: a dict from label bytes to index for the exact matches, ALL PAIRS of (miss,
label) for the neighbours -- no table, no hash, no candidates.  It also counts what a case exercises (corrected records,
ties, strict winners, barcodes without a neighbour, cells of corrected records only), so that the random cases can be held
to exercising the rule.  tests/test_correct_barcodes_gpu.py holds the device to the host walk on the same cases."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth, writers
from oarfish_amd import build as _b
from oarfish_amd.em import BarcodeRuleC, UmiRuleC, gather_names
from tests.test_dedup_umis import FILTERS, _input, pack

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "correct_barcodes_main.cpp")
EXE = os.path.join(HERE, "native", "correct_barcodes_main")
HDRS = [os.path.join(ROOT, "oarfish_amd", "csrc", h) for h in ("oem_barcode_correct.h", "oem_barcode_table.h")]
CORRECT = "oem_correct_barcodes"
ONE_CALL = "oem_em_run_cells_records_whitelist_sparse"
HOOK = "oem_test_correct_barcodes_host"
EXACT, CORRECTED, NO_NEIGHBOUR, AMBIGUOUS, MISSING = range(5)
NO_ID = 0xFFFFFFFF
ACGT = b"ACGT"


# ---------------------------------------------------------------------------------------------------------------------
# the walk and the cases
# ---------------------------------------------------------------------------------------------------------------------
def restate_rule(case, multi):
    """((id, status, order, cell_rec_off, counts) as lists, what the case exercised) from the rule as the issue states it."""
    wl, bcs, alphabet = case["whitelist"], case["barcodes"], case.get("alphabet", ACGT)
    index = {}
    for w, label in enumerate(wl):
        assert label not in index, "the case's whitelist repeats a label"
        index[label] = w
    n = len(bcs)
    ids, status, n_of = [NO_ID] * n, [None] * n, [0] * len(wl)
    for i, b in enumerate(bcs):
        if not b:
            status[i] = MISSING
        elif b in index:
            ids[i], status[i] = index[b], EXACT
            n_of[index[b]] += 1
    stats = dict(corrected=0, ties=0, strict=0, no_neighbour=0, corrected_only_cells=0, corrected_to_zero=0)
    for i, b in enumerate(bcs):
        if status[i] is not None:
            continue
        nb = []
        for w, label in enumerate(wl):                          # all pairs: every label against every miss
            if len(label) != len(b):
                continue
            diff = [p for p in range(len(b)) if label[p] != b[p]]
            if len(diff) == 1 and label[diff[0]] in alphabet:
                nb.append(w)
        if not nb:
            status[i] = NO_NEIGHBOUR
            stats["no_neighbour"] += 1
        elif len(nb) == 1:
            ids[i], status[i] = nb[0], CORRECTED
            stats["corrected_to_zero"] += n_of[nb[0]] == 0
        elif not multi:
            status[i] = AMBIGUOUS
        else:
            top = max(n_of[w] for w in nb)
            best = [w for w in nb if n_of[w] == top]
            if len(best) == 1:
                ids[i], status[i] = best[0], CORRECTED
                stats["strict"] += 1
            else:
                status[i] = AMBIGUOUS
                stats["ties"] += 1
        stats["corrected"] += status[i] == CORRECTED
    cell_of, members = {}, []
    for i in range(n):
        if ids[i] != NO_ID:
            if ids[i] not in cell_of:
                cell_of[ids[i]] = len(members)
                members.append([])
            members[cell_of[ids[i]]].append(i)
    order = [i for m in members for i in m]
    cro = [0]
    for m in members:
        cro.append(cro[-1] + len(m))
    stats["corrected_only_cells"] = sum(1 for m in members if all(status[i] == CORRECTED for i in m))
    counts = [sum(1 for s in status if s == k) for k in range(5)]
    return (ids, status, order, cro, counts), stats


L16 = b"ACGTACGTACGTACGT"


def _sub(b, pos, byte):
    return b[:pos] + bytes([byte]) + b[pos + 1:]


def hand_cases():
    """One case per sentence of the rule."""
    out = {}
    # an error at byte 0, 7, 8 and the last byte of a 16-byte label (two 8-byte words), and the label itself
    out["errors_at_word_edges"] = dict(whitelist=[L16, b"TTTTTTTTTTTTTTTT"],
                                       barcodes=[_sub(L16, p, ord("T") if L16[p] != ord("T") else ord("A")) for p in (0, 7, 8, 15)] + [L16])
    out["an_N_and_two_Ns"] = dict(whitelist=[L16, b"GGGGGGGGGGGGGGGG"],
                                  barcodes=[_sub(L16, 3, ord("N")), _sub(_sub(L16, 3, ord("N")), 9, ord("N")), b"NGGGGGGGGGGGGGGG", b"N" * 16])
    # the label's byte at the differing position must be in the alphabet; the barcode's own may be anything
    out["label_byte_outside_the_alphabet"] = dict(whitelist=[b"ACNT", b"AXGT", b"TTTT"],
                                                  barcodes=[b"ACGT", b"ACNT", b"ANGT", b"AXGT", b"AXGA", b"TTNT", b"TXTT", b"ACNA"])
    out["another_alphabet"] = dict(whitelist=[b"AXGT", b"ACNT", b"acgt"], alphabet=b"XNacgt",
                                   barcodes=[b"ACGT", b"AXGA", b"AcGT", b"Acgt", b"aCgt", b"ACNT", b"ACNG"])
    for length in (1, 7, 8, 9, 16, 17, 64):
        a = (L16 * 4)[:length]
        b = bytes(ACGT[(ACGT.index(x) + 1) % 4] for x in a)     # every position differs
        bcs = [a, b, _sub(a, length - 1, ord("N")), _sub(a, 0, b[0]), _sub(b, length // 2, ord("N")), a + b"A", a[:-1]]
        if length > 1:
            bcs.append(_sub(_sub(a, 0, ord("N")), length - 1, ord("N")))
        out[f"length_{length}"] = dict(whitelist=[a, b], barcodes=bcs)
    out["mixed_lengths_and_a_barcode_longer_than_every_label"] = dict(
        whitelist=[b"A", b"ACGTACG", b"ACGTACGT", b"ACGTACGTA", L16, L16 + b"A", (L16 * 4)],
        barcodes=[b"C", b"ACGTACC", b"ACGTACGA", b"ACGTACGTC", L16[:15] + b"A", L16 + b"C", (L16 * 4)[:63] + b"A", L16 * 4 + b"A",
                  L16 * 5, b"AC", L16[:10]])
    # AAAA and AATT are two apart: AATA / AAAT are neighbours of both
    pair = [b"AAAA", b"AATT", b"CCCC"]
    out["two_neighbours_with_a_strict_winner"] = dict(whitelist=pair, barcodes=[b"AAAA", b"AAAA", b"AATT", b"AATA", b"AAAT", b"CCCA"])
    out["two_neighbours_with_a_tie"] = dict(whitelist=pair, barcodes=[b"AAAA", b"AATT", b"AATA", b"AAAT", b"AATA"])
    out["two_neighbours_that_nobody_matches_exactly"] = dict(whitelist=pair, barcodes=[b"AATA", b"CCCC"])
    out["one_neighbour_with_n_0"] = dict(whitelist=pair, barcodes=[b"CCCA", b"CCCG", b"AAAA"])
    # corrected records never raise n: three corrected to AAAA leave n(AAAA) = 1 against n(AATT) = 2
    out["a_corrected_record_does_not_raise_n"] = dict(whitelist=pair,
                                                      barcodes=[b"AAAA", b"CAAA", b"GAAA", b"TAAA", b"AATT", b"AATT", b"AATA"])
    out["missing_barcodes"] = dict(whitelist=pair, barcodes=[b"", b"AAAA", b"", b"AAAC", b""])
    out["everything_rejected"] = dict(whitelist=pair, barcodes=[b"", b"GGGG", b"AATA", b"AAAAA", b"NNNN", b""])
    out["one_label"] = dict(whitelist=[b"ACGT"], barcodes=[b"ACGT", b"ACGA", b"AGGA", b"", b"NCGT", b"ACGT"])
    out["no_records"] = dict(whitelist=pair, barcodes=[])
    # rejected records first and last, a cell of corrected records only between exact cells, input order inside cells
    out["cells_in_order_of_their_first_accepted_record"] = dict(
        whitelist=[b"AAAA", b"CCCC", b"GGGG", b"TTTT"],
        barcodes=[b"", b"GGGA", b"TTTT", b"AAAA", b"GGGC", b"TTTA", b"AAAA", b"CCGG", b"GGGT", b"NNNN"])
    return out


def random_case(seed, n_labels=240, n_records=2600, length=12):
    """A whitelist with labels at distance 1 and 2 from each other and records of every kind: exact ones in uneven
    numbers (labels without any among them), single substitutions, the barcodes between two labels, Ns, garbage, gaps."""
    rng = np.random.default_rng([seed, 0xBC])
    wl = synth.make_whitelist(n_labels, length=length, seed=1000 + seed)
    labels = [wl[0][int(wl[1][w]):int(wl[1][w + 1])].tobytes() for w in range(n_labels)]
    known = set(labels)
    weight = rng.integers(0, 4, size=n_labels).astype(np.float64)          # a quarter of the labels has no exact record
    between, tied = [], []                                                 # barcodes one step from two labels
    for ia, a in enumerate(labels[:120]):
        for ib, b in enumerate(labels):
            diff = [p for p in range(length) if a[p] != b[p]]
            if len(diff) == 2:
                between.append(_sub(a, diff[0], b[diff[0]]))
                if len(tied) < 15:                                         # the two labels draw exact records alike ...
                    weight[ia] = weight[ib] = 0.0                          # ... none: a tie at n = 0
                    tied.append(between[-1])
    assert len(between) >= 20 and len(tied) >= 12
    weight /= weight.sum()
    bcs = []
    for _ in range(n_records):
        u, label = rng.random(), labels[int(rng.choice(n_labels, p=weight))]
        if u < 0.55:
            bcs.append(label)
        elif u < 0.75:                                                     # one substitution of any label, with or without exact records
            lab = labels[int(rng.integers(0, n_labels))]
            p = int(rng.integers(0, length))
            bcs.append(_sub(lab, p, ACGT[(ACGT.index(lab[p]) + int(rng.integers(1, 4))) % 4]))
        elif u < 0.87:
            bcs.append(between[int(rng.integers(0, len(between)))])
        elif u < 0.91:
            bcs.append(_sub(label, int(rng.integers(0, length)), ord("N")))
        elif u < 0.97:
            bcs.append(bytes(ACGT[k] for k in rng.integers(0, 4, size=length)))
        elif u < 0.98:
            bcs.append(label[:-1])
        else:
            bcs.append(b"")
    for k, b in enumerate(tied):                                           # every tie is in the input at least once
        bcs[(k * 97 + 13) % n_records] = b
    assert any(b in known for b in bcs)
    return dict(whitelist=labels, barcodes=bcs)


RANDOM_SEEDS = (1, 2)


def all_cases():
    """(label, case, multi) of everything the host walk and the device are compared on."""
    out = []
    for name, case in hand_cases().items():
        out += [(f"{name}, multi {m}", case, m) for m in (0, 1)]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# calling the C side
# ---------------------------------------------------------------------------------------------------------------------
def make_rule(case, multi, alphabet="case"):
    """(the oem_barcode_rule of a case, what it points into)."""
    blob, off = pack(case["whitelist"])
    if not len(blob):
        blob = np.zeros(1, dtype=np.uint8)
    alpha = case.get("alphabet") if alphabet == "case" else alphabet
    a = None if alpha is None else np.frombuffer(alpha, dtype=np.uint8).copy()
    rule = BarcodeRuleC(blob.ctypes.data, off.ctypes.data, len(case["whitelist"]), int(multi), None if a is None or not len(a) else a.ctypes.data,
                        0 if a is None else len(a), 0)
    return rule, (blob, off, a)


def call_correct(L, fn, case, multi, device=None, outs=True, rule=None):
    """oem_correct_barcodes (device = 0) or the hook (device = None): (rc, message, id, status, order, cell_rec_off, counts)."""
    keep = None
    if rule is None:
        rule, keep = make_rule(case, multi)
    blob, off = pack(case["barcodes"])
    n = len(case["barcodes"])
    if not len(blob):
        blob = np.zeros(1, dtype=np.uint8)
    ids = np.full(max(n, 1), 0xEEEEEEEE, dtype=np.uint32)
    status = np.full(max(n, 1), 0xEE, dtype=np.uint8)
    order = np.full(max(n, 1), 0xEEEEEEEE, dtype=np.uint32)
    cro = np.full(n + 1, 2 ** 64 - 1, dtype=np.uint64)
    counts = np.full(5, 2 ** 64 - 1, dtype=np.uint64)
    n_cells, n_acc = C.c_uint64(77), C.c_uint64(77)
    ptr = lambda a: a.ctypes.data if outs else None   # noqa: E731
    rc = getattr(L, fn)(C.addressof(rule) if rule else None, blob.ctypes.data if n else None, off.ctypes.data, n,
                        *([] if device is None else [device]), ptr(ids), ptr(status), ptr(order), ptr(cro), C.byref(n_cells), C.byref(n_acc),
                        ptr(counts))
    nc, na = int(n_cells.value), int(n_acc.value)
    del keep
    return rc, (L.oem_last_error() or b"").decode(), ids[:n].tolist(), status[:n].tolist(), order[:na].tolist(), cro[:nc + 1].tolist(), \
        counts.tolist()


def host_walk(case, multi):
    rc, msg, *got = call_correct(_lib.testing_lib(), HOOK, case, multi)
    assert rc == _lib.OEM_OK, msg
    return tuple(got)


# ---------------------------------------------------------------------------------------------------------------------
# declared, exported, bound
# ---------------------------------------------------------------------------------------------------------------------
def _declaration(name):
    src = open(os.path.join(ROOT, "include", "oarfish_em.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
    assert m, "include/oarfish_em.h does not declare " + name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,n_args,second,last", [(CORRECT, 12, "const uint8_t *barcodes", "uint64_t *out_counts"),
                                                     (ONE_CALL, 35, "const oem_umi_rule *umi_rule", "oem_cells_result **out")])
def test_declared_exported_by_both_libraries_and_bound(name, n_args, second, last):
    args = _declaration(name)
    assert len(args) == n_args and args[0] == "const oem_barcode_rule *rule" and args[1] == second and args[-1] == last
    for path in (_b.LIB_PATH, _b.TESTING_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert name in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, path
    assert name in _lib.ABI_SYMBOLS
    assert len(getattr(_lib.lib(), name).argtypes) == n_args
    assert len(getattr(_lib.testing_lib(), name).argtypes) == n_args
    assert _lib.lib().oem_abi_version() == 2
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = [ln for ln in doc.splitlines() if "`%s`" % name in ln and ln.lstrip().startswith("|")]
    assert row and "no counterpart" in row[0] and "docs/index.md:308-312" in row[0], "INTEGRATION.md has no row for it"
    assert HOOK in _b.TESTING_HOOKS and len(_lib.testing_lib().oem_test_correct_barcodes_host.argtypes) == 11
    out = subprocess.check_output(["nm", "-D", "--defined-only", _b.LIB_PATH], text=True)
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip()) == sorted(_b.header_symbols())
    assert C.sizeof(BarcodeRuleC) == 40
    hdr = open(os.path.join(ROOT, "include", "oarfish_em.h")).read()
    for k, word in enumerate(("EXACT", "CORRECTED", "NO_NEIGHBOUR", "AMBIGUOUS", "MISSING")):
        assert re.search(r"#define OEM_BARCODE_%s %d\b" % (word, k), hdr) and getattr(_lib, "OEM_BARCODE_" + word) == k
    assert "NEVER LOOKED AT" in hdr          # the header says what a rejected record's name, UMI and ref_id are


# ---------------------------------------------------------------------------------------------------------------------
# the host walk: the testing library's hook, and the stand-alone program under sanitizers
# ---------------------------------------------------------------------------------------------------------------------
def test_the_walk_itself():
    (ids, status, order, cro, counts), stats = restate_rule(hand_cases()["cells_in_order_of_their_first_accepted_record"], 0)
    assert ids == [NO_ID, 2, 3, 0, 2, 3, 0, NO_ID, 2, NO_ID]
    assert status == [MISSING, CORRECTED, EXACT, EXACT, CORRECTED, CORRECTED, EXACT, NO_NEIGHBOUR, CORRECTED, NO_NEIGHBOUR]
    assert order == [1, 4, 8, 2, 5, 3, 6] and cro == [0, 3, 5, 7] and counts == [3, 4, 2, 0, 1]
    assert stats["corrected_only_cells"] == 1 and stats["corrected_to_zero"] == 3
    cases = hand_cases()
    for multi, want in ((0, [0, 0, 1, NO_ID, NO_ID, 2]), (1, [0, 0, 1, 0, 0, 2])):
        assert restate_rule(cases["two_neighbours_with_a_strict_winner"], multi)[0][0] == want
    assert restate_rule(cases["two_neighbours_with_a_tie"], 1)[0][1] == [EXACT, EXACT, AMBIGUOUS, AMBIGUOUS, AMBIGUOUS]
    assert restate_rule(cases["a_corrected_record_does_not_raise_n"], 1)[0][0] == [0, 0, 0, 0, 1, 1, 1]
    assert restate_rule(cases["an_N_and_two_Ns"], 0)[0][1] == [CORRECTED, NO_NEIGHBOUR, CORRECTED, NO_NEIGHBOUR]
    got = restate_rule(cases["label_byte_outside_the_alphabet"], 0)[0]
    #             ACGT: ACNT's N is no alphabet byte; AXGT's X neither   ANGT -> nothing   AXGA -> AXGT (T is)   TTNT, TXTT -> TTTT
    assert got[0] == [NO_ID, 0, NO_ID, 1, 1, 2, 2, 0] and got[1][0] == NO_NEIGHBOUR
    assert restate_rule(cases["everything_rejected"], 1)[0][2:4] == ([], [0])
    assert restate_rule(cases["mixed_lengths_and_a_barcode_longer_than_every_label"], 0)[0][1] == [CORRECTED] * 7 + [NO_NEIGHBOUR] * 4


def test_the_host_walk_equals_the_walk_here():
    for label, case, multi in all_cases():
        assert host_walk(case, multi) == restate_rule(case, multi)[0], label


def test_the_default_alphabet_and_null_outputs():
    L = _lib.testing_lib()
    case = hand_cases()["cells_in_order_of_their_first_accepted_record"]
    want = restate_rule(case, 1)[0]
    rule, keep = make_rule(case, 1, alphabet=None)                    # alphabet NULL: ACGT
    rc, msg, *got = call_correct(L, HOOK, case, 1, rule=rule)
    assert rc == _lib.OEM_OK and tuple(got) == want, msg
    rc, msg, *got = call_correct(L, HOOK, case, 1, outs=False)        # every output but the two scalars NULL
    assert rc == _lib.OEM_OK and (len(got[2]), len(got[3]) - 1) == (7, 3), msg


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_the_host_walk_on_random_cases_that_exercise_the_rule(seed):
    case = random_case(seed)
    want, stats = restate_rule(case, 1)
    # asserted on the walk here, not on the code under test: the input must exercise every branch of the rule
    assert stats["corrected"] >= 100 and stats["ties"] >= 10 and stats["strict"] >= 10 and stats["no_neighbour"] >= 10, stats
    assert stats["corrected_only_cells"] >= 1, stats
    assert host_walk(case, 1) == want
    want0, stats0 = restate_rule(case, 0)
    assert want0 != want and want0[4][AMBIGUOUS] >= stats["ties"] + stats["strict"]
    assert host_walk(case, 0) == want0


def test_the_host_walk_with_short_hashes_and_a_small_first_table(monkeypatch):
    """The walk's table under the testing library's knobs: every label in the last slots, probes that wrap."""
    case = random_case(RANDOM_SEEDS[0], n_labels=80, n_records=500)
    want = restate_rule(case, 1)[0]
    for bits in ("0", "4"):
        monkeypatch.setenv("OEM_BARCODE_HASH_BITS", bits)
        monkeypatch.setenv("OEM_BARCODE_TABLE_SLOTS0", "2")
        assert host_walk(case, 1) == want, bits


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-o", EXE, SRC])
    return EXE


def _request(case, multi, hash_bits=64, slots0=8192):
    lines = [f"R {len(case['whitelist'])} {len(case['barcodes'])} {int(multi)} {case.get('alphabet', ACGT).hex() or '-'} {hash_bits} {slots0}"]
    lines += [w.hex() or "-" for w in case["whitelist"]]
    lines += [b.hex() or "-" for b in case["barcodes"]]
    return "\n".join(lines) + "\n"


def _walk(exe, requests):
    r = subprocess.run([exe], input="".join(requests), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[-1] == "" and len(out) == len(requests) + 1
    return out[:-1]


def test_the_host_walk_under_sanitizers(exe):
    cases = [(label, case, multi, 64, 8192) for label, case, multi in all_cases()]
    for seed in RANDOM_SEEDS:
        cases += [(f"random {seed}, multi {m}", random_case(seed), m, 64, 8192) for m in (0, 1)]
    small = random_case(RANDOM_SEEDS[1], n_labels=80, n_records=500)
    cases += [(f"short hashes: {bits} bits", small, 1, bits, 2) for bits in (0, 4)]
    for (label, case, multi, _, _), line in zip(cases, _walk(exe, [_request(c, m, b, s) for _, c, m, b, s in cases])):
        parts = [[int(x) for x in p.split()] for p in line.split("|")[1:]]
        assert line.startswith("ok") and len(parts) == 5, (label, line)
        assert tuple(parts) == restate_rule(case, multi)[0], label


def test_what_the_device_call_finds_is_found_by_the_walk(exe):
    L = _lib.testing_lib()
    good = [b"ACGT", b"AAAA"]
    zero_label = dict(whitelist=[b"ACGT", b"AC\x00T", b"\x00CGT"], barcodes=good)
    equal = dict(whitelist=[b"ACGT", b"TTTT", b"GGGG", b"TTTT", b"ACGT", b"TTTT"], barcodes=good)
    zero_barcode = dict(whitelist=[b"ACGT"], barcodes=[b"ACGT", b"", b"AC\x00T", b"\x00"])
    both = dict(whitelist=[b"ACGT", b"ACGT", b"A\x00"], barcodes=[b"\x00"])          # the label's 0 byte comes first
    for case, word, line in ((zero_label, "label 1 of the whitelist contains a 0 byte", "zerolabel 1"),
                             (equal, "labels 0 and 4 of the whitelist are equal", "equal 0 4"),
                             (zero_barcode, "the barcode of record 2 contains a 0 byte", "zerobarcode 2"),
                             (both, "label 2 of the whitelist contains a 0 byte", "zerolabel 2")):
        rc, msg, *_ = call_correct(L, HOOK, case, 0)
        assert rc == _lib.OEM_ERR_ARG and HOOK in msg and word in msg, msg
        assert _walk(exe, [_request(case, 0)]) == [line]
    assert host_walk(dict(whitelist=[b"ACGT"], barcodes=good), 0)[0] == [0, NO_ID]    # a good call after the errors


# ---------------------------------------------------------------------------------------------------------------------
# argument errors before any device use, and the wrappers
# ---------------------------------------------------------------------------------------------------------------------
def _bad_rules():
    """(what is wrong, the rule, what it points into, the message's words)."""
    blob, off = pack([b"ACGT", b"AAAA"])
    two, out = len(off) - 1, []
    acgt = np.frombuffer(ACGT, dtype=np.uint8).copy()

    def rule(labels=blob, label_off=off, n=two, multi=0, alphabet=None, n_alpha=0):
        ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
        return BarcodeRuleC(ptr(labels), ptr(label_off), n, multi, ptr(alphabet), n_alpha, 0)

    out.append(("labels NULL", rule(labels=None), "labels or rule->label_off is NULL"))
    out.append(("label_off NULL", rule(label_off=None), "labels or rule->label_off is NULL"))
    out.append(("no label", rule(n=0), "n_labels is 0"))
    for what, offs, word in (("not from 0", [1, 4, 8], "label_off must start at 0"), ("decreasing", [0, 5, 4], "non-decreasing (label 1)"),
                             ("an empty label", [0, 4, 4], "label 1 of the whitelist is empty")):
        o = np.array(offs, dtype=np.uint64)
        out.append((what, rule(label_off=o), word, o))
    long_blob, long_off = pack([b"ACGT", b"A" * 65])
    out.append(("a label of 65 bytes", rule(labels=long_blob, label_off=long_off), "label 1 of the whitelist has more than 64 bytes", long_blob, long_off))
    out.append(("multi = 2", rule(multi=2), "multi = 2 is neither 0 nor 1"))
    out.append(("an empty alphabet", rule(alphabet=acgt, n_alpha=0), "n_alphabet is 0"))
    nine = np.frombuffer(b"ACGTNacgt", dtype=np.uint8).copy()
    out.append(("an alphabet of nine", rule(alphabet=nine, n_alpha=9), "at most 8 bytes", nine))
    rep = np.frombuffer(b"ACGA", dtype=np.uint8).copy()
    out.append(("a repeated byte", rule(alphabet=rep, n_alpha=4), "byte 3 of rule->alphabet repeats", rep))
    zero = np.frombuffer(b"AC\x00T", dtype=np.uint8).copy()
    out.append(("a 0 byte", rule(alphabet=zero, n_alpha=4), "byte 2 of rule->alphabet is 0", zero))
    return out, (blob, off, acgt)


def test_rule_argument_errors_come_before_any_device_use():
    case = dict(whitelist=[b"ACGT", b"AAAA"], barcodes=[b"ACGT", b"ACGA"])
    bad, keep = _bad_rules()
    for L, fn, device in ((_lib.lib(), CORRECT, 0), (_lib.testing_lib(), CORRECT, 0), (_lib.testing_lib(), HOOK, None)):
        for what, rule, word, *_held in bad:
            rc, msg, *_ = call_correct(L, fn, case, 0, device=device, rule=rule)
            assert rc == _lib.OEM_ERR_ARG and fn in msg and word in msg, (what, msg)
        rc, msg, *_ = call_correct(L, fn, case, 0, device=device, rule=False)
        assert rc == _lib.OEM_ERR_ARG and "the barcode rule is NULL" in msg, msg
        # the limits and checks of oem_collate_barcodes on the input side
        rule, held = make_rule(case, 0)
        out = [np.zeros(8, dtype=np.uint64) for _ in range(7)]
        u64p = lambda a: C.cast(a.ctypes.data, C.POINTER(C.c_uint64))   # noqa: E731
        outs = [o.ctypes.data for o in out[:4]] + [u64p(out[4]), u64p(out[5]), out[6].ctypes.data]
        blob, off = pack(case["barcodes"])
        dev = [] if device is None else [device]
        for n, offs, word in ((2 ** 32, off, "more than 2^32 - 1"), (2 ** 31 - 1, off, "at most 2^31 - 2"),
                              (2, np.array([1, 4, 8], dtype=np.uint64), "barcode_off must start at 0"),
                              (2, np.array([0, 5, 4], dtype=np.uint64), "non-decreasing (record 1)")):
            rc = getattr(L, fn)(C.addressof(rule), blob.ctypes.data, offs.ctypes.data, n, *dev, *outs)
            assert rc == _lib.OEM_ERR_ARG and word.encode() in L.oem_last_error(), (n, L.oem_last_error())
        rc = getattr(L, fn)(C.addressof(rule), None, off.ctypes.data, 2, *dev, *outs)
        assert rc == _lib.OEM_ERR_ARG and b"barcodes is NULL" in L.oem_last_error()
        rc = getattr(L, fn)(C.addressof(rule), blob.ctypes.data, off.ctypes.data, 2, *dev, *outs[:4], None, outs[5], None)
        assert rc == _lib.OEM_ERR_ARG and b"out_n_cells or out_n_accepted is NULL" in L.oem_last_error()
        rc = getattr(L, fn)(C.addressof(rule), blob.ctypes.data, None, 2, *dev, *outs)
        assert rc == _lib.OEM_ERR_ARG and b"barcode_off, out_n_cells or out_n_accepted is NULL" in L.oem_last_error()
    rc, msg, *_ = call_correct(_lib.lib(), CORRECT, case, 0, device=0)
    if _lib.device_count() == 0:
        assert rc == _lib.OEM_ERR_NO_DEVICE, msg
    else:
        assert rc == _lib.OEM_OK, msg
    del keep


def _one_call(L, rule, umi_rule, a, n_txps=40, n=5):
    res = C.c_void_p(1)
    ptr = lambda x: None if x is None else x.ctypes.data   # noqa: E731
    rc = getattr(L, ONE_CALL)(C.addressof(rule) if rule else None, None if umi_rule is None else C.addressof(umi_rule), C.addressof(a["F"]),
                              ptr(a["tl"]), n_txps, ptr(a["rec"]), n, ptr(a["bc_blob"]), ptr(a["bc_off"]), ptr(a["blob"]), ptr(a["off"]),
                              ptr(a["sec"]), ptr(a["um_blob"]), ptr(a["um_off"]), 0, 100, -1, 2.0, 0, 100, 1e-3,
                              *([None] * 13), C.byref(res))
    return rc, res, L.oem_last_error() or b""


def test_one_call_argument_errors_come_before_any_device_use():
    L = _lib.lib()
    a = _input()
    barcodes = [a["bc_blob"][int(a["bc_off"][i]):int(a["bc_off"][i + 1])].tobytes() for i in range(5)]
    good, keep = make_rule(dict(whitelist=sorted(set(barcodes))), 0)
    bad, keep2 = _bad_rules()
    for what, rule, word, *_held in bad:
        rc, res, msg = _one_call(L, rule, None, a)
        assert rc == _lib.OEM_ERR_ARG and not res.value and word.encode() in msg and ONE_CALL.encode() in msg, (what, msg)
    rc, res, msg = _one_call(L, False, None, a)
    assert rc == _lib.OEM_ERR_ARG and not res.value and b"the barcode rule is NULL" in msg
    # ... beside the UMI rule's and the umis call's own
    rc, res, msg = _one_call(L, good, UmiRuleC(None, 0, 2), a)
    assert rc == _lib.OEM_ERR_ARG and not res.value and b"correct = 2" in msg and ONE_CALL.encode() in msg
    rc, res, msg = _one_call(L, good, None, dict(a, um_off=None))
    assert rc == _lib.OEM_ERR_ARG and not res.value and b"umis is given and umi_off is NULL" in msg
    rc, res, msg = _one_call(L, good, None, dict(a, off=None))
    assert rc == _lib.OEM_ERR_ARG and not res.value and b"name_off is NULL" in msg
    for umis in (True, False):                    # umis / umi_off may both be NULL: no deduplication
        rc, res, msg = _one_call(L, good, None, a if umis else dict(a, um_blob=None, um_off=None))
        if _lib.device_count() > 0:
            assert rc == _lib.OEM_OK and res.value, msg
            L.oem_cells_result_destroy(res)
        else:
            assert rc == _lib.OEM_ERR_NO_DEVICE and not res.value, (rc, msg)
    del keep, keep2


def test_the_wrappers_check_their_own_arguments():
    a = _input()
    names, barcodes = (a["blob"], a["off"]), (a["bc_blob"], a["bc_off"])
    run = lambda **kw: oarfish_amd.em_cells_records_sparse(FILTERS, a["tl"], a["rec"], None, None, names=names, **kw)   # noqa: E731
    for collate in ("host", "device"):
        with pytest.raises(ValueError, match="whitelist goes with barcodes"):
            run(whitelist=[b"ACGT"], collate=collate)
        with pytest.raises(ValueError, match="barcode_multi goes with whitelist"):
            run(barcodes=barcodes, barcode_multi=True, collate=collate)
        with pytest.raises(ValueError, match="whitelist needs one label"):
            run(barcodes=barcodes, whitelist=[], collate=collate)
    with pytest.raises(ValueError, match="whitelist needs one label"):
        oarfish_amd.correct_barcodes([b"ACGT"], [])
    for alphabet in (b"", b"ACGTNacgt"):
        with pytest.raises(ValueError, match="alphabet needs 1 to 8 bytes"):
            oarfish_amd.correct_barcodes([b"ACGT"], [b"ACGT"], alphabet=alphabet)
    with pytest.raises(_lib.OemError) as e:                           # what the wrapper leaves to the call
        oarfish_amd.correct_barcodes([b"ACGT"], [b"ACGT", b""])
    assert e.value.code == _lib.OEM_ERR_ARG and "label 1 of the whitelist is empty" in str(e.value)
    with pytest.raises(_lib.OemError) as e:
        oarfish_amd.correct_barcodes([b"ACGT"], [b"ACGT"], alphabet=b"AA")
    assert e.value.code == _lib.OEM_ERR_ARG and "repeats" in str(e.value)
    assert {"correct_barcodes", "add_barcode_errors", "make_whitelist"} <= set(oarfish_amd.__all__)
    assert writers.cell_labels([b"AAAA", b"CCCC", b"GG"], [NO_ID, 2, 0, 2, NO_ID, 1], [1, 3, 2, 5], [0, 2, 3, 4]) == ["GG", "AAAA", "CCCC"]
    with pytest.raises(ValueError, match="has no label"):
        writers.cell_labels([b"AAAA"], [NO_ID, 0], [0, 1], [0, 2])
    if _lib.device_count() == 0:
        with pytest.raises(_lib.OemError) as e:
            oarfish_amd.correct_barcodes([b"ACGT", b"ACGA"], [b"ACGT"], multi=True)
        assert e.value.code == _lib.OEM_ERR_NO_DEVICE
        for collate in ("host", "device"):
            with pytest.raises(oarfish_amd.OemError) as e:
                run(barcodes=barcodes, whitelist=[b"ACGT", b"AAAA"], barcode_multi=True, collate=collate)
            assert e.value.code == _lib.OEM_ERR_NO_DEVICE


# ---------------------------------------------------------------------------------------------------------------------
# the synthetic whitelist and errors
# ---------------------------------------------------------------------------------------------------------------------
def _strings(pair):
    raw, off = np.asarray(pair[0]).tobytes(), np.asarray(pair[1]).astype(np.int64)
    return [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def test_make_whitelist():
    wl = synth.make_whitelist(400, seed=3)
    labels = _strings(wl)
    assert wl[0].dtype == np.uint8 and wl[1].dtype == np.uint64 and len(labels) == 400 == len(set(labels))
    assert all(len(x) == 16 and set(x) <= set(ACGT) for x in labels)
    dist = {1: 0, 2: 0}
    for i, a in enumerate(labels):
        for b in labels[i + 1:]:
            d = sum(x != y for x, y in zip(a, b))
            if d in dist:
                dist[d] += 1
    assert dist[1] >= 20 and dist[2] >= 20, dist
    assert _strings(synth.make_whitelist(400, seed=3)) == labels and _strings(synth.make_whitelist(400, seed=4)) != labels
    assert sorted(_strings(synth.make_whitelist(4, length=1))) == [b"A", b"C", b"G", b"T"]
    assert len(set(_strings(synth.make_whitelist(50, length=40)))) == 50
    with pytest.raises(ValueError):
        synth.make_whitelist(5, length=1)


def test_add_barcode_errors_hits_the_records_of_a_read_alike():
    rng = np.random.default_rng(6)
    cells = _strings(synth.make_whitelist(7, seed=9))
    n_reads = 900
    read_cell = rng.integers(0, 7, size=n_reads)
    read_of = rng.integers(0, n_reads, size=3000)
    names = pack([b"read%d" % r for r in read_of])
    barcodes = pack([cells[read_cell[r]] if r % 50 else b"" for r in read_of])
    before = _strings(barcodes)
    out = synth.add_barcode_errors(barcodes, 0.2, 0.05, seed=8, names=names)
    assert _strings(barcodes) == before                                        # the input is left alone
    after = _strings(out)
    assert np.array_equal(out[1], barcodes[1]) and out[1].dtype == np.uint64
    per_read, subs, ns = {}, 0, 0
    for r, u, v in zip(read_of, before, after):
        diff = [p for p in range(len(u)) if u[p] != v[p]]
        assert len(u) == len(v) and len(diff) <= 1 and set(v) <= set(b"ACGTN")
        assert per_read.setdefault(int(r), v) == v                            # the same on all records of a read
    for r, v in per_read.items():
        if v and v != cells[read_cell[r]]:
            ns += b"N" in v
            subs += b"N" not in v
    n_hit = sum(1 for v in per_read.values() if v)
    assert 0.12 * n_hit < subs < 0.28 * n_hit and 0.02 * n_hit < ns < 0.09 * n_hit, (subs, ns, n_hit)
    # a pure function, of the read and the seed and not of the records' order
    assert _strings(synth.add_barcode_errors(barcodes, 0.2, 0.05, seed=8, names=names)) == after
    assert _strings(synth.add_barcode_errors(barcodes, 0.2, 0.05, seed=9, names=names)) != after
    perm = rng.permutation(3000)
    assert _strings(synth.add_barcode_errors(gather_names(barcodes, perm), 0.2, 0.05, seed=8, names=gather_names(names, perm))) == \
        [after[i] for i in perm]
    assert _strings(synth.add_barcode_errors(barcodes, 0.0, names=names)) == before
    assert sum(x != y for x, y in zip(_strings(synth.add_barcode_errors(barcodes, 0.0, 1.0)), before)) == sum(1 for u in before if u)
    with pytest.raises(ValueError):
        synth.add_barcode_errors(barcodes, 0.7, 0.7)
