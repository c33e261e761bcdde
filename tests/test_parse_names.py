"""CPU tests of the bulk parser on the device (oem_store_create_records_names): declared, exported by both libraries,
bound with the header's argument count, every host-visible argument error before any device use, the synthetic input,
and the host walk of the rule (oarfish_amd/csrc/oem_collate.h, parse_bulk_host) in a stand-alone program under the
address and undefined-behaviour sanitizers, held to the oracle below.

The oracle is pure Python and knows nothing of the C++ walk.  Under ADJACENT it transcribes alignment_parser.rs:361-427
literally: the ``prev_read`` state machine, a set for the collation check, ``rg_num``.  (The set is a dict here so that
the oracle can also name the earlier group's first record, which the reference's message does not.)  Under SORT it is
``sorted`` over (name bytes, secondary, index) of the surviving records and the same cut.
tests/test_records_names_gpu.py holds the device to the same oracle on the same cases."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth
from oarfish_amd import build as _b
from oarfish_amd.builder import ALN_RECORD, filters_c
from oarfish_amd.types import DeviceStore
from tests.test_collate import ADJACENT, SORT, pack

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "parse_bulk_main.cpp")
EXE = os.path.join(HERE, "native", "parse_bulk_main")
HDR = os.path.join(ROOT, "oarfish_amd", "csrc", "oem_collate.h")
NAME = "oem_store_create_records_names"
UNMAPPED = _lib.REC_UNMAPPED
T = 40
FILTERS = dict(five_prime_clip=2 ** 32 - 1, three_prime_clip=2 ** 62, score_threshold=0.95, min_aligned_fraction=0.5,
               min_aligned_len=50, which_strand=0, score_prob_denom=5.0)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
class NotCollated(Exception):
    def __init__(self, group, record, earlier):
        super().__init__(group, record, earlier)
        self.group, self.record, self.earlier = group, record, earlier


class BadName(Exception):
    def __init__(self, record, zero_byte):
        super().__init__(record, zero_byte)
        self.record, self.zero_byte = record, zero_byte


def oracle(unmapped, names, sec, mode, check):
    """dict(order, group_off, n_unmapped, n_parsed, n_groups, n_checked); raises BadName or NotCollated (which carries
    the same dict as ``.parsed``).  unmapped: flags; names: bytes per record; sec: flags or None."""
    n = len(names)
    survivors = [i for i in range(n) if not unmapped[i]]
    for i in survivors:
        if not names[i] or 0 in names[i]:
            raise BadName(i, 0 in names[i])
    groups, error = [], None
    if mode == ADJACENT:   # alignment_parser.rs:361-427
        read_name_map, rg_num, prev_read, records_for_read = {}, 0, b"", []
        for i in range(n):
            if unmapped[i]:
                continue
            rstring = names[i]
            if prev_read == rstring:
                records_for_read.append(i)
            else:
                if prev_read:
                    groups.append(records_for_read)
                    records_for_read = []
                prev_read = rstring
                if rg_num < check:
                    if prev_read in read_name_map and error is None:
                        error = NotCollated(len(groups), i, read_name_map[prev_read])   # (the walk goes on: the test wants the groups too)
                    read_name_map.setdefault(prev_read, i)
                    rg_num += 1
                records_for_read.append(i)
        if records_for_read:
            groups.append(records_for_read)
        n_checked = rg_num
    else:
        idx = sorted(survivors, key=lambda i: (names[i], bool(sec[i]) if sec is not None else False, i))
        for k, i in enumerate(idx):
            if k == 0 or names[i] != names[idx[k - 1]]:
                groups.append([])
            groups[-1].append(i)
        n_checked = 0
    order = [i for g in groups for i in g]
    group_off = [0]
    for g in groups:
        group_off.append(group_off[-1] + len(g))
    out = dict(order=order, group_off=group_off, n_unmapped=n - len(survivors), n_parsed=len(survivors), n_groups=len(groups),
               n_checked=n_checked)
    if error is not None:
        error.parsed = out
        raise error
    return out


def test_the_oracle_itself():
    A, B = b"readA", b"readB"
    got = oracle([0, 1, 0], [A, b"", A], None, ADJACENT, 10)
    assert got["order"] == [0, 2] and got["group_off"] == [0, 2] and got["n_unmapped"] == 1 and got["n_checked"] == 1
    assert oracle([0, 1, 0], [A, B, A], None, ADJACENT, 10)["group_off"] == [0, 2]          # an unmapped record named B cuts nothing
    with pytest.raises(NotCollated) as e:
        oracle([0, 0, 0], [A, B, A], None, ADJACENT, 10)
    assert (e.value.group, e.value.record, e.value.earlier) == (2, 2, 0)
    assert oracle([0, 0, 0], [A, B, A], None, ADJACENT, 2)["group_off"] == [0, 1, 2, 3]    # the repeat is group N: accepted
    assert oracle([0, 0, 0], [A, B, A], None, ADJACENT, 0)["n_checked"] == 0
    got = oracle([0, 0, 0, 1], [B, A, B, A], [1, 0, 0, 0], SORT, 10)
    assert got["order"] == [1, 2, 0] and got["group_off"] == [0, 1, 3] and got["n_checked"] == 0
    assert oracle([1, 1], [b"", b"\0"], None, ADJACENT, 10) == dict(order=[], group_off=[0], n_unmapped=2, n_parsed=0, n_groups=0, n_checked=0)
    with pytest.raises(BadName) as e:
        oracle([1, 0, 0], [b"", b"x\0", b""], None, SORT, 10)
    assert (e.value.record, e.value.zero_byte) == (1, True)


# ---------------------------------------------------------------------------------------------------------------------
# the cases both tiers run: name -> (unmapped flags, names, secondary or None, mode, sort_check_num)
# ---------------------------------------------------------------------------------------------------------------------
def _reads(names_and_sizes):
    return [nm for nm, k in names_and_sizes for _ in range(k)]


def parse_cases():
    base = bytes(range(0x41, 0x41 + 26))
    cases = {}
    for mode, tag in ((ADJACENT, "adjacent"), (SORT, "sort")):
        cases[f"empty input/{tag}"] = ([], [], None, mode, 10)
        cases[f"all unmapped/{tag}"] = ([1, 1, 1], [b"a", b"", b"\0\0"], None, mode, 10)
        cases[f"unmapped first/{tag}"] = ([1, 0, 0, 0], [b"zz", b"r1", b"r1", b"r2"], None, mode, 10)
        cases[f"unmapped last/{tag}"] = ([0, 0, 0, 1], [b"r1", b"r1", b"r2", b"r2"], None, mode, 10)
        cases[f"unmapped inside a read/{tag}"] = ([0, 1, 0, 0], [b"r1", b"r1", b"r1", b"r2"], None, mode, 10)
        cases[f"unmapped inside a read, named otherwise/{tag}"] = ([0, 1, 0, 0], [b"r1", b"r2", b"r1", b"r2"], None, mode, 10)
        cases[f"unmapped with an empty name and with a 0 byte/{tag}"] = ([0, 1, 1, 0, 0], [b"r1", b"", b"a\0b", b"r1", b"r2"], None, mode, 10)
        lens = [base[:k] for k in (1, 7, 8, 9, 15, 16, 17)]
        cases[f"name lengths/{tag}"] = ([0] * 14, _reads([(nm, 2) for nm in lens]), [0, 1] * 7, mode, 100)
        cases[f"proper prefixes/{tag}"] = ([0] * 7, _reads([(b"ACGTACGTAC", 2), (b"ACGT", 1), (b"ACGTACGT", 3), (b"ACGTACGTA", 1)]),
                                           None, mode, 100)
        cases[f"N above the groups/{tag}"] = ([0] * 6, _reads([(b"r%d" % k, 2) for k in range(3)]), None, mode, 10 ** 9)
        cases[f"N = 0/{tag}"] = ([0] * 5, [b"a", b"b", b"a", b"c", b"b"], None, mode, 0)
        # a repeat among the checked groups: group 0's name again at group N - 1, and exactly at group N (accepted)
        names = [b"g%d" % k for k in range(8)]
        cases[f"repeat of group 0 at group N - 1/{tag}"] = ([0] * 8, names[:5] + [names[0]] + names[6:], None, mode, 6)
        cases[f"repeat of group 0 exactly at group N/{tag}"] = ([0] * 8, names[:5] + [names[0]] + names[6:], None, mode, 5)
        cases[f"two repeats, the smaller group wins/{tag}"] = ([0] * 8, [b"a", b"b", b"c", b"b", b"d", b"a", b"e", b"a"], None, mode, 8)
        cases[f"repeat behind unmapped records/{tag}"] = ([1, 0, 1, 0, 0, 1], [b"", b"a", b"a", b"b", b"a", b"b"], None, mode, 8)
    rng = np.random.default_rng(77)
    pool = [base[:k] for k in (1, 2, 7, 8, 9, 16, 17)] + [b"A00741:132:HJ3KVDSX2:1:1101:%d:%d" % (x, x * 7) for x in range(1000, 1012)]
    for k in range(200):   # collated runs of a few names, unmapped records sprinkled in, now and then a repeated name
        n_reads = int(rng.integers(0, 40))
        picks = rng.permutation(len(pool))[:min(n_reads, len(pool))] if rng.random() < 0.7 else rng.integers(0, len(pool), size=n_reads)
        names, unm, sec = [], [], []
        for p in picks:
            for j in range(int(rng.integers(1, 5))):
                if rng.random() < 0.2:
                    names.append([b"", b"\0", pool[int(rng.integers(0, len(pool)))]][int(rng.integers(0, 3))])
                    unm.append(1)
                    sec.append(0)
                names.append(pool[int(p)])
                unm.append(0)
                sec.append(int(j > 0 and rng.random() < 0.8))
        names, unm, sec = names[:300], unm[:300], sec[:300]
        mode = SORT if k % 3 == 0 else ADJACENT
        check = [0, 1, 3, 10, 100_000][int(rng.integers(0, 5))]
        cases[f"random {k}"] = (unm, names, sec if k % 2 else None, mode, check)
    return cases


def bad_name_cases():
    """(unmapped, names, the first bad surviving record, whether it is a 0 byte)"""
    good = [b"read%02d" % (i // 2) for i in range(40)]
    out = []
    for at in (0, 17, 39):
        for bad, zero in ((b"", 0), (b"ACGTACGT\0C", 1), (b"\0", 1)):
            names, unm = list(good), [0] * 40
            names[at] = bad
            if at == 17:
                names[30] = b"" if zero else b"A\0"      # a later bad one of the other kind does not win
                names[5], unm[5] = b"", 1                # an earlier bad one on an unmapped record is never looked at
                names[6], unm[6] = b"\0", 1
            out.append((unm, names, at, zero))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# declared, exported, bound
# ---------------------------------------------------------------------------------------------------------------------
def test_declared_exported_by_both_libraries_and_bound():
    src = open(os.path.join(ROOT, "include", "oarfish_em.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, src)
    assert m, "include/oarfish_em.h does not declare " + NAME
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 23 and args[0] == "const oem_filters *filters" and args[-1] == "oem_store **out"
    assert "oem_parse_info" in src
    for path in (_b.LIB_PATH, _b.TESTING_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert NAME in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, path
    assert NAME in _lib.ABI_SYMBOLS
    assert len(getattr(_lib.lib(), NAME).argtypes) == 23 and len(getattr(_lib.testing_lib(), NAME).argtypes) == 23
    assert _lib.lib().oem_abi_version() == 2
    assert C.sizeof(_lib.ParseInfoC) == 64
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = [ln for ln in doc.splitlines() if NAME in ln and ln.lstrip().startswith("|")]
    assert row and "alignment_parser.rs:301-437" in row[0], "INTEGRATION.md has no row for it"


# ---------------------------------------------------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------------------------------------------------
def _input():
    rec = np.zeros(6, dtype=ALN_RECORD)
    for i in range(6):
        rec[i] = (i % T, 10, 1500, 1400, 1000 - i, 1500, _lib.REC_HAS_SCORE, 0)
    rec["flags"][2] = UNMAPPED
    blob, off = pack([b"r1", b"r1", b"", b"r1", b"q", b"q"])
    return dict(F=filters_c(FILTERS), tl=np.full(T, 2000, dtype=np.uint64), rec=rec, blob=blob, off=off,
                sec=np.array([0, 1, 0, 1, 0, 1], dtype=np.uint8))


def _call(L, F, tl, rec, blob, off, sec, n_txps=T, n=6, mode=ADJACENT, check=100_000, bin_width=100, model=-1, opts=None, out=True,
          rows=(False, False)):
    res = C.c_void_p(1)
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    row_blob, row_off = np.zeros(64, dtype=np.uint8), np.zeros(8, dtype=np.uint64)
    rc = getattr(L, NAME)(None if F is None else C.addressof(F), ptr(tl), n_txps, ptr(rec), n, ptr(blob), ptr(off), ptr(sec), mode, check,
                          bin_width, model, 2.0, 0, None if opts is None else C.addressof(opts), None, None, None,
                          row_blob.ctypes.data if rows[0] else None, row_off.ctypes.data if rows[1] else None, None, None,
                          C.byref(res) if out else None)
    return rc, res, L.oem_last_error() or b""


def test_argument_errors_come_before_any_device_use():
    L = _lib.lib()
    a = _input()

    def moved(off, at, v):
        off = off.copy()
        off[at] = v
        return off

    def opts(field, v):
        o = _lib.StoreOptsC()
        setattr(o, field, v)
        return o

    cases = [   # (what is wrong, arguments, a word of the message): the records call's, the names', this call's own
        ("filters NULL", dict(F=None), b"bad argument"),
        ("txp_len NULL", dict(tl=None), b"bad argument"),
        ("n_txps 0", dict(n_txps=0), b"bad argument"),
        ("model 2", dict(model=2), b"model"),
        ("model -2", dict(model=-2), b"model"),
        ("bin width 0 with a model", dict(model=1, bin_width=0), b"bin width"),
        ("weight_coding 3", dict(opts=opts("weight_coding", 3)), b"weight_coding"),
        ("layout_build 2", dict(opts=opts("layout_build", 2)), b"layout_build"),
        ("reorder_rows 3", dict(opts=opts("reorder_rows", 3)), b"reorder_rows"),
        ("records NULL", dict(rec=None), b"records is NULL"),
        ("names NULL", dict(blob=None), b"names is NULL"),
        ("name_off NULL", dict(off=None), b"NULL"),
        ("name_off not from 0", dict(off=moved(a["off"], 0, 1)), b"name_off must start at 0"),
        ("name_off decreases", dict(off=moved(a["off"], 2, 1)), b"name_off must be non-decreasing (record 1)"),
        ("too many records", dict(n=2 ** 31 - 1), b"2^31 - 2"),
        ("no such mode", dict(mode=2), b"mode"),
        ("row names without their offsets", dict(rows=(True, False)), b"out_row_names and out_row_name_off"),
        ("row name offsets without the names", dict(rows=(False, True)), b"out_row_names and out_row_name_off"),
    ]
    for what, kw, word in cases:
        b = dict(a)
        b.update(kw)
        rc, res, msg = _call(L, **b)
        assert rc == _lib.OEM_ERR_ARG, (what, rc, msg)
        assert not res.value, what
        assert word in msg and NAME.encode() in msg or word == b"bin width" and word in msg, (what, msg)
    rc, _, msg = _call(L, **a, out=False)
    assert rc == _lib.OEM_ERR_ARG and b"out is NULL" in msg


def test_well_formed_input_needs_a_device():
    L = _lib.lib()
    a = _input()
    for mode in (SORT, ADJACENT):
        for model in (-1, 0, 1):
            rc, res, msg = _call(L, **a, mode=mode, model=model, rows=(True, True))
            if _lib.device_count() > 0:
                assert rc == _lib.OEM_OK and res.value, msg
                L.oem_store_destroy(res)
            else:
                assert rc == _lib.OEM_ERR_NO_DEVICE and not res.value, (rc, msg)
    if _lib.device_count() == 0:
        with pytest.raises(oarfish_amd.OemError) as e:
            DeviceStore.from_named_records(FILTERS, a["tl"], a["rec"], (a["blob"], a["off"]), secondary=a["sec"])
        assert e.value.code == _lib.OEM_ERR_NO_DEVICE


def test_the_wrapper_checks_its_own_arguments():
    a = _input()
    names = (a["blob"], a["off"])
    with pytest.raises(ValueError, match="mode"):
        DeviceStore.from_named_records(FILTERS, a["tl"], a["rec"], names, mode="sorted")
    with pytest.raises(ValueError, match="names must have one entry per record"):
        DeviceStore.from_named_records(FILTERS, a["tl"], a["rec"][:5], names)
    with pytest.raises(ValueError, match="secondary must have one entry per record"):
        DeviceStore.from_named_records(FILTERS, a["tl"], a["rec"], names, secondary=a["sec"][:5])
    with pytest.raises(ValueError, match="coverage model"):
        DeviceStore.from_named_records(FILTERS, a["tl"], a["rec"], names, coverage="kde")


# ---------------------------------------------------------------------------------------------------------------------
# the synthetic input
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style", ["uuid", "illumina"])
def test_make_named_records(style):
    sr = synth.make_records(synth.make_store(300, 40, seed=5), seed=6)
    n, G = len(sr.records), len(sr.group_off) - 1
    rec, (blob, off), sec = synth.make_named_records(sr, style=style, seed=9)
    assert np.array_equal(rec, sr.records) and len(off) == n + 1 and len(sec) == n
    names = [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(n)]
    per_group = [names[int(sr.group_off[g])] for g in range(G)]
    assert len(set(per_group)) == G and all(nm and 0 not in nm for nm in names)
    for g in range(G):
        a, b = int(sr.group_off[g]), int(sr.group_off[g + 1])
        assert set(names[a:b]) == {per_group[g]} and sec[a] == 0 and all(sec[a + 1:b] == 1)
    # extra unmapped records, inside and between the reads, with and without a name; the mapped input is untouched
    sr0 = synth.make_records(synth.make_store(300, 40, seed=5), seed=6, drop_frac=0.0)      # (no unmapped records of its own)
    n0 = len(sr0.records)
    rec0, (blob0, off0), _ = synth.make_named_records(sr0, style=style, seed=9)
    rec2, (blob2, off2), sec2 = synth.make_named_records(sr0, style=style, seed=9, unmapped_rate=0.2)
    names2 = [bytes(blob2[int(off2[i]):int(off2[i + 1])]) for i in range(len(rec2))]
    extra = (rec2["flags"] & UNMAPPED) != 0
    assert extra.sum() == len(rec2) - n0 == round(0.2 * n0) and not sec2[extra].any()
    assert np.array_equal(rec2[~extra], sr0.records)
    assert [names2[i] for i in np.flatnonzero(~extra)] == [bytes(blob0[int(off0[i]):int(off0[i + 1])]) for i in range(n0)]
    ours = np.flatnonzero(extra)
    assert any(names2[i] == b"" for i in ours) and any(names2[i] for i in ours)
    assert not {names2[i] for i in ours if names2[i]} & {names2[i] for i in np.flatnonzero(~extra)}
    assert sum(1 for i in ours if 0 < i < len(rec2) - 1 and not extra[i - 1] and not extra[i + 1] and names2[i - 1] == names2[i + 1]) > 0
    assert sum(1 for i in ours if 0 < i < len(rec2) - 1 and not extra[i - 1] and not extra[i + 1] and names2[i - 1] != names2[i + 1]) > 0
    # shuffled: a permutation of the same multiset, and a pure function of its arguments
    rec3, (blob3, off3), sec3 = synth.make_named_records(sr0, style=style, seed=9, unmapped_rate=0.2, shuffle=True)
    names3 = [bytes(blob3[int(off3[i]):int(off3[i + 1])]) for i in range(len(rec3))]
    assert sorted(names3) == sorted(names2) and names3 != names2 and sorted(rec3["score"].tolist()) == sorted(rec2["score"].tolist())
    again = synth.make_named_records(sr0, style=style, seed=9, unmapped_rate=0.2, shuffle=True)
    assert np.array_equal(again[0], rec3) and np.array_equal(again[1][0], blob3) and np.array_equal(again[2], sec3)
    assert not np.array_equal(synth.make_named_records(sr0, style=style, seed=10, unmapped_rate=0.2)[1][0], blob2)


# ---------------------------------------------------------------------------------------------------------------------
# oem_collate.h's bulk rule, stand-alone, under sanitizers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-o", EXE, SRC])
    return EXE


def _request(unm, names, sec, mode, check):
    lines = [f"P {len(names)} {mode} {check}"]
    for i, nm in enumerate(names):
        lines.append(f"{UNMAPPED if unm[i] else 0} {int(sec[i]) if sec is not None else 0} {nm.hex() or '-'}")
    return "\n".join(lines) + "\n"


def _walk(exe, requests):
    r = subprocess.run([exe], input="".join(requests), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[-1] == "" and len(out) == len(requests) + 1
    return out[:-1]


def expected_line(unm, names, sec, mode, check):
    """What the stand-alone program prints for a case, from the oracle."""
    def body(p):
        return (f"{p['n_unmapped']} {p['n_parsed']} {p['n_groups']} {p['n_checked']} |" + "".join(f" {i}" for i in p["order"]) + " |"
                + "".join(f" {o}" for o in p["group_off"]))
    try:
        return "ok " + body(oracle(unm, names, sec, mode, check))
    except NotCollated as e:
        p = dict(e.parsed)
        p["n_checked"] = min(check, p["n_groups"])      # (the reference stops at the repeat; the rule counts the groups it checks)
        return f"repeat {e.group} {e.record} {e.earlier} " + body(p)
    except BadName as e:
        return f"bad {e.record} {int(e.zero_byte)}"


def test_host_walk_matches_the_oracle_under_sanitizers(exe):
    cases = parse_cases()
    answers = _walk(exe, [_request(*c) for c in cases.values()])
    n_repeat = 0
    for (name, c), line in zip(cases.items(), answers):
        assert line == expected_line(*c), name
        n_repeat += line.startswith("repeat")
    assert n_repeat >= 10 and sum(a.startswith("ok") for a in answers) >= 100      # both verdicts are exercised
    assert answers[list(cases).index("repeat of group 0 at group N - 1/adjacent")].startswith("repeat 5 5 0 ")
    assert answers[list(cases).index("repeat of group 0 exactly at group N/adjacent")].startswith("ok ")
    assert answers[list(cases).index("two repeats, the smaller group wins/adjacent")].startswith("repeat 3 3 1 ")
    assert answers[list(cases).index("repeat behind unmapped records/adjacent")].startswith("repeat 2 4 1 ")
    assert answers[list(cases).index("unmapped inside a read, named otherwise/adjacent")] == "ok 1 3 2 2 | 0 2 3 | 0 2 3"


def test_host_walk_reports_the_first_bad_surviving_name(exe):
    cases = bad_name_cases()
    for mode in (ADJACENT, SORT):
        got = _walk(exe, [_request(unm, names, None, mode, 100) for unm, names, _, _ in cases])
        assert got == [f"bad {at} {zero}" for _, _, at, zero in cases]
