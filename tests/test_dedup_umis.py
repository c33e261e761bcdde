"""CPU tests of UMI deduplication (oem_dedup_umis, oem_em_run_cells_records_umis_sparse): declared, exported by both
libraries and bound; the host walk of the rule (oarfish_amd/csrc/oem_collate.h, dedup_umis_host) against a restatement
written here; the same walk in a stand-alone program under the address and undefined-behaviour sanitizers; every
host-visible argument error before any device use; the Python wrappers' own checks; the synthetic duplicates.

The restatement knows nothing of the C++ walk: per cell a dict keyed by the UMI's bytes, filled in group order, so the
first group of a class is its survivor.  tests/test_dedup_umis_gpu.py holds the device to the host walk on the same cases."""
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
from tests.test_collate import ADJACENT, SORT, pack as _pack

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "dedup_umis_main.cpp")
EXE = os.path.join(HERE, "native", "dedup_umis_main")
HDR = os.path.join(ROOT, "oarfish_amd", "csrc", "oem_collate.h")
DEDUP = "oem_dedup_umis"
ONE_CALL = "oem_em_run_cells_records_umis_sparse"
UNMAPPED = _lib.REC_UNMAPPED
T = 40
FILTERS = dict(five_prime_clip=2 ** 32 - 1, three_prime_clip=2 ** 62, score_threshold=0.95, min_aligned_fraction=0.5,
               min_aligned_len=50, which_strand=0, score_prob_denom=5.0)


def pack(strings):
    return _pack(strings) if len(strings) and any(len(s) for s in strings) else \
        (np.zeros(0, dtype=np.uint8), np.zeros(len(strings) + 1, dtype=np.uint64))


# ---------------------------------------------------------------------------------------------------------------------
# the restatement and the cases
# ---------------------------------------------------------------------------------------------------------------------
def restate(case):
    """(dup, survivor, cell_dups) as lists, from the rule as the issue states it."""
    umis, flags, order, goff, cgo = case["umis"], case["flags"], case["order"], case["group_off"], case["cell_group_off"]
    ng, nc = len(goff) - 1, len(cgo) - 1
    dup, survivor, cell_dups = [0] * ng, list(range(ng)), [0] * nc
    for c in range(nc):
        first = {}
        for g in range(cgo[c], cgo[c + 1]):
            if goff[g + 1] == goff[g]:
                continue
            head = order[goff[g]]
            if not umis[head] or (flags is not None and flags[head] & UNMAPPED):
                continue
            if umis[head] in first:
                dup[g], survivor[g] = 1, first[umis[head]]
                cell_dups[c] += 1
            else:
                first[umis[head]] = g
    return dup, survivor, cell_dups


def restate_drop(case, dup):
    order, goff, cgo = case["order"], case["group_off"], case["cell_group_off"]
    o2, g2, c2, r2 = [], [0], [], []
    for c in range(len(cgo) - 1):
        c2.append(len(g2) - 1)
        r2.append(len(o2))
        for g in range(cgo[c], cgo[c + 1]):
            if not dup[g]:
                o2 += order[goff[g]:goff[g + 1]]
                g2.append(len(o2))
    return o2, g2, c2 + [len(g2) - 1], r2 + [len(o2)]


def make_case(cells, seed=0, with_flags=True):
    """cells: a list of cells, a cell a list of groups, a group a list of records ``umi`` or ``(umi, flags)``, in collated
    order.  The records get their input indices from a seeded permutation, so ``order`` is no identity."""
    recs = [r if isinstance(r, tuple) else (r, 0) for cell in cells for group in cell for r in group]
    n = len(recs)
    perm = np.random.default_rng(seed).permutation(n).tolist() if seed is not None else list(range(n))
    umis, flags = [b""] * n, [0] * n
    for k, (u, f) in enumerate(recs):
        umis[perm[k]], flags[perm[k]] = u, f
    goff, cgo = [0], [0]
    for cell in cells:
        for group in cell:
            goff.append(goff[-1] + len(group))
        cgo.append(len(goff) - 1)
    return dict(umis=umis, flags=flags if with_flags else None, order=perm, group_off=goff, cell_group_off=cgo)


def umi_cases():
    """name -> case (make_case's dict)."""
    base = b"ACGTACGTTGCATGCAA"     # 17 bytes: two whole keys and a byte
    x, y = b"AACCGGTTAACC", b"TTGGCCAATTGG"
    cases = {}
    cases["no_groups"] = make_case([])
    cases["no_groups_one_cell"] = make_case([[]])
    cases["one_group"] = make_case([[[x, x]]])
    cases["all_distinct"] = make_case([[[b"UMI%05d" % (i * 7919 % 1000)] * (1 + i % 3) for i in range(40)]], seed=1)
    cases["one_class_is_a_whole_cell"] = make_case([[[x]] * 9], seed=2)
    cases["same_umi_in_two_cells"] = make_case([[[x], [y]], [[x], [y, y]]], seed=3)
    cases["proper_prefix"] = make_case([[[b"ACG"], [b"ACGT"], [b"ACG", b"ACG"], [b"ACGT"], [b"A"]]], seed=4)
    lens = [base[:n] for n in (8, 9, 16, 17)]
    cases["keys_of_8_9_16_17_bytes"] = make_case([[[lens[i]] for i in (0, 1, 2, 3, 3, 2, 1, 0, 2, 0)]], seed=5)
    cases["empty_umis_between_class_members"] = make_case([[[x], [b""], [x], [b"", x], [b""], [x, b""]]], seed=6)
    cases["unmapped_head_before_its_mapped_twin"] = make_case([[[(x, UNMAPPED)], [x], [x], [(y, UNMAPPED), y], [y]]], seed=7)
    cases["unmapped_without_flags"] = make_case([[[(x, UNMAPPED)], [x], [x]]], seed=7, with_flags=False)
    cases["non_head_record_with_another_umi"] = make_case([[[x, y], [y], [x], [y, x]]], seed=8)
    cases["an_empty_cell"] = make_case([[[x], [x]], [], [[x], [y], [x]], []], seed=9)
    cases["a_group_without_records"] = make_case([[[x], [], [x], []], [[], [y]]], seed=9)
    cases["three_cells_every_second_group_a_duplicate"] = make_case(
        [[[b"M%03d" % (g // 2)] * (1 + g % 2) for g in range(2 * k)] for k in (5, 64, 33)], seed=10)
    cases["identity_order"] = make_case([[[x], [y], [x]], [[y], [y]]], seed=None)
    return cases


def test_the_restatement_itself():
    c = make_case([[[b"A"], [b"B"], [b"A"], [b"A"]], [[b"A"]]], seed=None)
    assert restate(c) == ([0, 0, 1, 1, 0], [0, 1, 0, 0, 4], [2, 0])
    assert restate_drop(c, [0, 0, 1, 1, 0]) == ([0, 1, 4], [0, 1, 2, 3], [0, 2, 3], [0, 2, 3])
    c = make_case([[[(b"A", UNMAPPED)], [b"A"], [b"AB"], [b""], [b""]]], seed=None)
    assert restate(c) == ([0] * 5, list(range(5)), [0])
    cases = umi_cases()
    assert sum(restate(cases["three_cells_every_second_group_a_duplicate"])[0]) == 5 + 64 + 33
    assert restate(cases["unmapped_head_before_its_mapped_twin"])[0] == [0, 0, 1, 0, 0]
    assert restate(cases["unmapped_without_flags"])[0] == [0, 1, 1]
    assert restate(cases["non_head_record_with_another_umi"])[:2] == ([0, 0, 1, 1], [0, 1, 0, 1])
    assert restate(cases["keys_of_8_9_16_17_bytes"])[2] == [6]


# ---------------------------------------------------------------------------------------------------------------------
# declared, exported, bound
# ---------------------------------------------------------------------------------------------------------------------
def _declaration(name):
    src = open(os.path.join(ROOT, "include", "oarfish_em.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
    assert m, "include/oarfish_em.h does not declare " + name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,n_args,first,last", [(DEDUP, 14, "const uint8_t *umis", "uint64_t *out_cell_dups"),
                                                    (ONE_CALL, 29, "const oem_filters *filters", "oem_cells_result **out")])
def test_declared_exported_by_both_libraries_and_bound(name, n_args, first, last):
    args = _declaration(name)
    assert len(args) == n_args and args[0] == first and args[-1] == last
    for path in (_b.LIB_PATH, _b.TESTING_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert name in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, path
    assert name in _lib.ABI_SYMBOLS
    assert len(getattr(_lib.lib(), name).argtypes) == n_args
    assert len(getattr(_lib.testing_lib(), name).argtypes) == n_args
    assert _lib.lib().oem_abi_version() == 2
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = [ln for ln in doc.splitlines() if name in ln and ln.lstrip().startswith("|")]
    assert row and "no counterpart" in row[0] and "docs/index.md:308-312" in row[0], "INTEGRATION.md has no row for it"
    assert "oem_test_dedup_umis_host" in _b.TESTING_HOOKS


def test_the_product_exports_the_header_and_the_header_is_c99(tmp_path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _b.LIB_PATH], text=True)
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip()) == sorted(_b.header_symbols())
    src = tmp_path / "c99.c"
    src.write_text('#include "oarfish_em.h"\nint main(void) { return (int)sizeof(oem_aln_record) - 40; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "c99.o")])


# ---------------------------------------------------------------------------------------------------------------------
# the host walk: the testing library's hook, and the stand-alone program under sanitizers
# ---------------------------------------------------------------------------------------------------------------------
def call_dedup(L, fn, case, device=None, n_records=None):
    """oem_dedup_umis (device = 0) or the hook (device = None) on a case: (rc, message, dup, survivor, cell_dups)."""
    blob, off = pack(case["umis"])
    n = len(case["umis"]) if n_records is None else n_records
    order = np.array(case["order"], dtype=np.uint32)
    goff, cgo = np.array(case["group_off"], dtype=np.uint64), np.array(case["cell_group_off"], dtype=np.uint64)
    flags = None if case["flags"] is None else np.array(case["flags"], dtype=np.uint32)
    ng, nc = len(goff) - 1, len(cgo) - 1
    dup = np.full(max(ng, 1), 0xEE, dtype=np.uint8)
    survivor = np.full(max(ng, 1), 2 ** 64 - 1, dtype=np.uint64)
    cell_dups = np.full(max(nc, 1), 2 ** 64 - 1, dtype=np.uint64)
    if not len(blob):
        blob = np.zeros(1, dtype=np.uint8)
    head = [blob.ctypes.data, off.ctypes.data, None if flags is None or not len(flags) else flags.ctypes.data, n,
            order.ctypes.data if len(order) else None, len(order), goff.ctypes.data, ng, cgo.ctypes.data, nc]
    rc = getattr(L, fn)(*head, *([] if device is None else [device]), dup.ctypes.data, survivor.ctypes.data, cell_dups.ctypes.data)
    return rc, (L.oem_last_error() or b"").decode(), dup[:ng].tolist(), survivor[:ng].tolist(), cell_dups[:nc].tolist()


def host_walk(case):
    rc, msg, *got = call_dedup(_lib.testing_lib(), "oem_test_dedup_umis_host", case)
    assert rc == _lib.OEM_OK, msg
    return tuple(got)


def test_the_host_walk_equals_the_restatement():
    for name, case in umi_cases().items():
        assert host_walk(case) == restate(case), name


def test_the_host_walk_on_random_collations():
    rng = np.random.default_rng(12)
    for trial in range(30):
        pool = [bytes(rng.integers(0x41, 0x45, size=int(rng.integers(0, 4))).astype(np.uint8)) for _ in range(6)]
        cells = [[[(pool[int(rng.integers(0, 6))], int(rng.integers(0, 4) == 0)) for _ in range(int(rng.integers(0, 4)))]
                  for _ in range(int(rng.integers(0, 12)))] for _ in range(int(rng.integers(0, 5)))]
        case = make_case(cells, seed=trial)
        assert host_walk(case) == restate(case), trial


def test_the_hook_refuses_what_the_device_call_refuses():
    L = _lib.testing_lib()
    case = make_case([[[b"AC"], [b"A\x00C"], [b"AC"]], [[b"\x00"]]], seed=None)
    rc, msg, *_ = call_dedup(L, "oem_test_dedup_umis_host", case)
    assert rc == _lib.OEM_ERR_ARG and "the UMI of record 1 contains a 0 byte" in msg
    case = make_case([[[b"AC"], [b"AC"]]], seed=None)
    case["order"] = [0, 2]
    rc, msg, *_ = call_dedup(L, "oem_test_dedup_umis_host", case)
    assert rc == _lib.OEM_ERR_ARG and "order[1] = 2 is not below n_records = 2" in msg


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-o", EXE, SRC])
    return EXE


def _request(case):
    n, flags = len(case["umis"]), case["flags"]
    lines = [f"D {n} {len(case['order'])} {len(case['group_off']) - 1} {len(case['cell_group_off']) - 1} {int(flags is not None)}"]
    lines += [f"{u.hex() or '-'} {0 if flags is None else flags[i]}" for i, u in enumerate(case["umis"])]
    lines += [" ".join(str(v) for v in case[k]) for k in ("order", "group_off", "cell_group_off")]
    return "\n".join(lines) + "\n"


def _walk(exe, requests):
    r = subprocess.run([exe], input="".join(requests), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[-1] == "" and len(out) == len(requests) + 1
    return out[:-1]


def test_the_host_walk_and_the_drop_under_sanitizers(exe):
    cases = umi_cases()
    for (name, case), line in zip(cases.items(), _walk(exe, [_request(c) for c in cases.values()])):
        parts = [[int(x) for x in p.split()] for p in line.split("|")[1:]]
        assert line.startswith("ok") and len(parts) == 7, (name, line)
        dup, survivor, cell_dups = restate(case)
        assert tuple(parts[:3]) == (dup, survivor, cell_dups), name
        assert tuple(parts[3:]) == restate_drop(case, dup), name
        # ... and the NumPy compaction of the package is the same drop
        got = oarfish_amd.drop_groups(np.array(case["order"], dtype=np.uint32), case["group_off"], case["cell_group_off"], dup)
        assert tuple(a.tolist() for a in got) == restate_drop(case, dup), name
        assert got[0].dtype == np.uint32 and all(a.dtype == np.uint64 for a in got[1:])


def test_the_stand_alone_walk_reports_the_first_umi_with_a_0_byte(exe):
    bad = [make_case([[[b"AC"], [b"A\x00C"], [b"AC"]], [[b"\x00"]]], seed=None), make_case([[[b"ACGTACGT\x00"]]], seed=None)]
    assert _walk(exe, [_request(c) for c in bad]) == ["bad 1", "bad 0"]


# ---------------------------------------------------------------------------------------------------------------------
# argument errors before any device use, and no device
# ---------------------------------------------------------------------------------------------------------------------
def _dedup_input():
    blob, off = pack([b"AC", b"G", b"AC", b"", b"G"])
    return dict(blob=blob, off=off, flags=np.zeros(5, dtype=np.uint32), n=5, order=np.array([0, 2, 1, 3, 4], dtype=np.uint32), m=5,
                goff=np.array([0, 1, 2, 4, 5], dtype=np.uint64), ng=4, cgo=np.array([0, 2, 4], dtype=np.uint64), nc=2)


def _dedup_call(L, blob, off, flags, n, order, m, goff, ng, cgo, nc, outs=(True, True, True)):
    dup, survivor, cell_dups = np.zeros(8, dtype=np.uint8), np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    rc = L.oem_dedup_umis(ptr(blob), ptr(off), ptr(flags), n, ptr(order), m, ptr(goff), ng, ptr(cgo), nc, 0,
                          dup.ctypes.data if outs[0] else None, survivor.ctypes.data if outs[1] else None,
                          cell_dups.ctypes.data if outs[2] else None)
    return rc, L.oem_last_error() or b"", (dup[:ng].tolist(), survivor[:ng].tolist(), cell_dups[:nc].tolist())


def _moved(a, at, v):
    a = a.copy()
    a[at] = v
    return a


def test_dedup_argument_errors_come_before_any_device_use():
    L = _lib.lib()
    a = _dedup_input()
    cases = [   # (what is wrong, arguments, a word of the message)
        ("umis NULL", dict(blob=None), b"umis is NULL"),
        ("umi_off NULL", dict(off=None), b"NULL"),
        ("order NULL", dict(order=None), b"order is NULL"),
        ("group_off NULL", dict(goff=None), b"NULL"),
        ("cell_group_off NULL", dict(cgo=None), b"NULL"),
        ("umi_off not from 0", dict(off=_moved(a["off"], 0, 1)), b"umi_off must start at 0"),
        ("umi_off decreases", dict(off=_moved(a["off"], 2, 1)), b"umi_off must be non-decreasing (record 1)"),
        ("group_off not from 0", dict(goff=_moved(a["goff"], 0, 1)), b"group_off must start at 0"),
        ("group_off decreases", dict(goff=_moved(a["goff"], 2, 0)), b"group_off must be non-decreasing (group 1)"),
        ("group_off does not end at n_positions", dict(m=6), b"group_off ends at 5, not at n_positions = 6"),
        ("cell_group_off not from 0", dict(cgo=_moved(a["cgo"], 0, 1)), b"cell_group_off must start at 0"),
        ("cell_group_off decreases", dict(cgo=_moved(a["cgo"], 1, 5)), b"cell_group_off must be non-decreasing (cell 1)"),
        ("cell_group_off does not end at n_groups", dict(cgo=_moved(a["cgo"], 2, 3)), b"cell_group_off ends at 3, not at n_groups = 4"),
        ("too many records", dict(n=2 ** 32), b"2^32 - 1"),
    ]
    for what, kw, word in cases:
        b = dict(a)
        b.update(kw)
        rc, msg, _ = _dedup_call(L, **b)
        assert rc == _lib.OEM_ERR_ARG, (what, rc, msg)
        assert word in msg and DEDUP.encode() in msg, (what, msg)
    for k in range(3):
        rc, msg, _ = _dedup_call(L, **a, outs=tuple(j != k for j in range(3)))
        assert rc == _lib.OEM_ERR_ARG and b"NULL" in msg and DEDUP.encode() in msg, (k, rc, msg)


def _input():
    """Five records of three barcodes, interleaved; records 0 and 2 are one molecule read twice."""
    rec = np.zeros(5, dtype=ALN_RECORD)
    for i in range(5):
        rec[i] = (i % T, 10, 1500, 1400, 1000 - i, 1500, _lib.REC_HAS_SCORE, 0)
    blob, off = pack([b"r2", b"r1", b"r3", b"q", b"q"])
    bc_blob, bc_off = pack([b"AC", b"G", b"AC", b"TTT", b"G"])
    um_blob, um_off = pack([b"AAT", b"CC", b"AAT", b"", b"G"])
    return dict(F=filters_c(FILTERS), tl=np.full(T, 2000, dtype=np.uint64), rec=rec, bc_blob=bc_blob, bc_off=bc_off, blob=blob, off=off,
                sec=np.array([0, 0, 0, 0, 1], dtype=np.uint8), um_blob=um_blob, um_off=um_off)


def _call(L, F, tl, rec, bc_blob, bc_off, blob, off, sec, um_blob, um_off, n_txps=T, n=5, mode=SORT, bin_width=100, model=-1, out=True):
    res = C.c_void_p(1)
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    rc = getattr(L, ONE_CALL)(None if F is None else C.addressof(F), ptr(tl), n_txps, ptr(rec), n, ptr(bc_blob), ptr(bc_off), ptr(blob),
                              ptr(off), ptr(sec), ptr(um_blob), ptr(um_off), mode, bin_width, model, 2.0, 0, 100, 1e-3, None, None, None,
                              None, None, None, None, None, None, C.byref(res) if out else None)
    return rc, res, L.oem_last_error() or b""


def test_one_call_argument_errors_come_before_any_device_use():
    L = _lib.lib()
    a = _input()
    cases = [   # the barcodes call's, and the UMIs'
        ("filters NULL", dict(F=None), b"bad argument"),
        ("txp_len NULL", dict(tl=None), b"bad argument"),
        ("n_txps 0", dict(n_txps=0), b"bad argument"),
        ("model 2", dict(model=2), b"model"),
        ("bin width 0 with a model", dict(model=1, bin_width=0), b"bin width"),
        ("records NULL", dict(rec=None), b"records is NULL"),
        ("barcodes NULL", dict(bc_blob=None), b"barcodes is NULL"),
        ("barcode_off NULL", dict(bc_off=None), b"NULL"),
        ("barcode_off decreases", dict(bc_off=_moved(a["bc_off"], 2, 1)), b"barcode_off must be non-decreasing (record 1)"),
        ("names NULL", dict(blob=None), b"names is NULL"),
        ("name_off not from 0", dict(off=_moved(a["off"], 0, 1)), b"name_off must start at 0"),
        ("umis NULL", dict(um_blob=None), b"umis is NULL"),
        ("umi_off NULL", dict(um_off=None), b"umi_off is NULL"),
        ("umi_off not from 0", dict(um_off=_moved(a["um_off"], 0, 1)), b"umi_off must start at 0"),
        ("umi_off decreases", dict(um_off=_moved(a["um_off"], 2, 1)), b"umi_off must be non-decreasing (record 1)"),
        ("too many records", dict(n=2 ** 32), b"2^32 - 1"),
        ("no such mode", dict(mode=2), b"mode"),
    ]
    for what, kw, word in cases:
        b = dict(a)
        b.update(kw)
        rc, res, msg = _call(L, **b)
        assert rc == _lib.OEM_ERR_ARG, (what, rc, msg)
        assert not res.value, what
        assert word in msg and ONE_CALL.encode() in msg or word == b"bin width" and word in msg, (what, msg)
    rc, _, msg = _call(L, **a, out=False)
    assert rc == _lib.OEM_ERR_ARG and b"out is NULL" in msg


def test_well_formed_input_needs_a_device():
    L = _lib.lib()
    rc, msg, got = _dedup_call(L, **_dedup_input())
    if _lib.device_count() > 0:
        assert rc == _lib.OEM_OK, msg
        assert got == ([0, 1, 0, 1], [0, 0, 2, 2], [1, 1])      # AC, AC in the first cell; G (its head), G in the second
    else:
        assert rc == _lib.OEM_ERR_NO_DEVICE, (rc, msg)
        with pytest.raises(_lib.OemError) as e:
            oarfish_amd.dedup_umis([b"AC", b"AC"], [0, 1], [0, 1, 2], [0, 2])
        assert e.value.code == _lib.OEM_ERR_NO_DEVICE
    a = _input()
    for mode in (SORT, ADJACENT):
        for model in (-1, 0, 1):
            rc, res, msg = _call(L, **a, mode=mode, model=model)
            if _lib.device_count() > 0:
                assert rc == _lib.OEM_OK and res.value, msg
                L.oem_cells_result_destroy(res)
            else:
                assert rc == _lib.OEM_ERR_NO_DEVICE and not res.value, (rc, msg)
    if _lib.device_count() == 0:
        for collate in ("host", "device"):
            with pytest.raises(oarfish_amd.OemError) as e:
                oarfish_amd.em_cells_records_sparse(FILTERS, a["tl"], a["rec"], None, None, names=(a["blob"], a["off"]), secondary=a["sec"],
                                                    barcodes=(a["bc_blob"], a["bc_off"]), umis=(a["um_blob"], a["um_off"]), collate=collate)
            assert e.value.code == _lib.OEM_ERR_NO_DEVICE


def test_the_wrappers_check_their_own_arguments():
    a = _input()
    names, barcodes, umis = (a["blob"], a["off"]), (a["bc_blob"], a["bc_off"]), (a["um_blob"], a["um_off"])
    run = lambda *p, **kw: oarfish_amd.em_cells_records_sparse(FILTERS, a["tl"], *p, **kw)   # noqa: E731
    cro = np.array([0, 2, 4, 5], dtype=np.uint64)
    for collate in ("host", "device"):
        with pytest.raises(ValueError, match="umis goes with barcodes"):
            run(a["rec"], None, cro, names=names, umis=umis, collate=collate)
        with pytest.raises(ValueError, match="umis goes with barcodes"):
            run(a["rec"], cro, cro, umis=umis, collate=collate)
        with pytest.raises(ValueError, match="umis must have one entry per record"):
            run(a["rec"], None, None, names=names, barcodes=barcodes, umis=[b"A"] * 4, collate=collate)
        with pytest.raises(ValueError, match="needs names"):
            run(a["rec"], None, None, barcodes=barcodes, umis=umis, collate=collate)
    with pytest.raises(ValueError, match="flags must have one entry per record"):
        oarfish_amd.dedup_umis(umis, [0, 1], [0, 1, 2], [0, 2], flags=np.zeros(4, dtype=np.uint32))
    with pytest.raises(ValueError, match="dup must have one entry per group"):
        oarfish_amd.drop_groups([0, 1], [0, 1, 2], [0, 2], [0])
    assert {"dedup_umis", "drop_groups", "add_umi_duplicates"} <= set(oarfish_amd.__all__)


# ---------------------------------------------------------------------------------------------------------------------
# the synthetic duplicates
# ---------------------------------------------------------------------------------------------------------------------
def _synthetic_input(seed=3):
    rng = np.random.default_rng(seed)
    cro = np.array([0, 60, 61, 61, 150, 400], dtype=np.uint64)
    n = 400
    cell_of = np.repeat(np.arange(5), np.diff(cro.astype(np.int64)))
    names = [b"read%d/%d" % (cell_of[i], v) for i, v in enumerate(rng.integers(0, 60, size=n))]
    rec = np.zeros(n, dtype=ALN_RECORD)
    rec["ref_id"] = np.arange(n)
    rec["flags"] = np.where(rng.integers(0, 10, size=n) == 0, UNMAPPED, 0)
    sec = rng.integers(0, 2, size=n).astype(np.uint8)
    barcodes = synth.make_barcodes(5, "var", seed=2)
    r2, n2, s2, bc, _ = synth.interleave_cells(rec, pack(names), sec, cro, barcodes, seed=9)
    return r2, n2, s2, bc


def _strings(pair):
    blob, off = np.asarray(pair[0]), np.asarray(pair[1]).astype(np.int64)
    raw = blob.tobytes()
    return [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def test_add_umi_duplicates():
    rec, names, sec, bc = _synthetic_input()
    out = synth.add_umi_duplicates(rec, names, sec, bc, rate=0.3, seed=5)
    again = synth.add_umi_duplicates(rec, names, sec, bc, rate=0.3, seed=5)
    other = synth.add_umi_duplicates(rec, names, sec, bc, rate=0.3, seed=6)
    r2, n2, s2, b2, umis, copies = out
    assert all(np.array_equal(x, y) for x, y in zip((r2, *n2, s2, *b2, *umis), (again[0], *again[1], again[2], *again[3], *again[4])))
    assert copies == again[5] and not np.array_equal(umis[0], other[4][0])
    n, n_aug = len(rec), len(r2)
    assert n_aug > n and len(s2) == n_aug and len(n2[1]) == len(b2[1]) == len(umis[1]) == n_aug + 1
    nm, bcs, um = _strings(n2), _strings(b2), _strings(umis)
    assert all(len(u) == 12 and set(u) <= set(b"ACGT") for u in um)
    fresh = np.array([b"~" in x for x in nm])
    # the originals are the input, in its order
    assert np.array_equal(r2[~fresh], rec) and np.array_equal(s2[~fresh], sec)
    assert [x for x, f in zip(nm, fresh) if not f] == _strings(names) and [x for x, f in zip(bcs, fresh) if not f] == _strings(bc)
    # one UMI per read, and among the original reads of a cell no UMI twice
    umi_of, reads_of = {}, {}
    for k in range(n_aug):
        assert umi_of.setdefault((bcs[k], nm[k]), um[k]) == um[k]
    for (b, name), u in umi_of.items():
        if b"~" not in name:
            reads_of.setdefault((b, u), []).append(name)
    assert all(len(v) == 1 for v in reads_of.values())
    # a copy is its read again: the same records, flags, barcode and UMI under a fresh name, 1 to 3 times; no unmapped record
    by_read = {}
    for k in range(n_aug):
        by_read.setdefault((bcs[k], nm[k]), []).append(k)
    n_copies = {}
    for (b, name), idx in by_read.items():
        if b"~" not in name:
            continue
        orig = by_read[(b, name.rsplit(b"~", 1)[0])]
        assert umi_of[(b, name)] == umi_of[(b, name.rsplit(b"~", 1)[0])]
        key = lambda i: (r2[i].tobytes(), int(s2[i]))   # noqa: E731
        assert sorted(map(key, idx)) == sorted(map(key, orig)) and not (r2["flags"][idx] & UNMAPPED).any()
        n_copies[(b, name.rsplit(b"~", 1)[0])] = n_copies.get((b, name.rsplit(b"~", 1)[0]), 0) + 1
    assert set(n_copies.values()) <= {1, 2, 3} and len(set(n_copies.values())) > 1
    # the copy counts add up, per barcode and in all
    per_bc = {}
    for (b, _), k in n_copies.items():
        per_bc[b] = per_bc.get(b, 0) + k
    assert per_bc == copies and sum(copies.values()) == len([1 for key in by_read if b"~" in key[1]])
    n_reads = len([1 for key in by_read if b"~" not in key[1]])
    assert 0.15 * n_reads < len(n_copies) < 0.4 * n_reads
    # the copies are spread over the input, not appended
    assert fresh[:n_aug // 2].any() and fresh[n_aug // 2:].any() and not fresh[-(n_aug - n):].all()
    # rate 0: nothing is added
    r0 = synth.add_umi_duplicates(rec, names, None, bc, rate=0.0, seed=5)
    assert np.array_equal(r0[0], rec) and r0[2] is None and r0[5] == {} and _strings(r0[1]) == _strings(names)
    with pytest.raises(ValueError):
        synth.add_umi_duplicates(rec, names, sec, bc, rate=1.5)
