"""CPU tests of the gene rule -- oem_cells_gene_counts: declared, exported by both libraries and bound; the host walk of the
rule (oarfish_amd/csrc/oem_gene_counts.h, gene_counts_host) through the testing library's hook and in a stand-alone
program under the address and undefined-behaviour sanitizers, against a walk written here; every argument error before
any device use, with the index it names; the Python wrapper's own checks.

The walk here knows nothing of the C++ one: per cell a dict from gene to an ``np.float64`` that the entries are added to
one by one in CSR order, the genes sorted, ``np.float32`` of the sum.  (Not ``np.add.reduceat``: NumPy's float reductions
go pairwise from eight terms.)  tests/test_gene_counts_gpu.py holds the device to the host walk and to this walk on the
same cases."""
import ctypes as C
import os
import subprocess
import warnings

import numpy as np
import pytest

from oarfish_amd import _lib
from oarfish_amd import build as _b
from oarfish_amd.em import _take_cells_result, cells_gene_counts

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "gene_counts_main.cpp")
EXE = os.path.join(HERE, "native", "gene_counts_main")
HDR = os.path.join(ROOT, "oarfish_amd", "csrc", "oem_gene_counts.h")
ENTRY = "oem_cells_gene_counts"
HOOK = "oem_test_cells_gene_counts_host"
F32_MAX = np.float32(3.4028234663852886e38)


# ---------------------------------------------------------------------------------------------------------------------
# the walk of this file, and the cases
# ---------------------------------------------------------------------------------------------------------------------
def walk(indptr, cols, vals, gene_of, reverse=False, acc_type=np.float64):
    """(indptr_g, genes, vals_g) by the rule.  ``reverse`` and ``acc_type`` are the alternatives the value cases tell
    apart: the entries of a run taken backwards, an f32 accumulator."""
    out_off, genes, out = [0], [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # f32 max twice overflows to +inf on purpose
        for c in range(len(indptr) - 1):
            acc = {}
            es = range(int(indptr[c]), int(indptr[c + 1]))
            for e in (reversed(es) if reverse else es):
                g = int(gene_of[int(cols[e])])
                acc[g] = acc_type(acc.get(g, acc_type(0.0)) + acc_type(vals[e]))
            for g in sorted(acc):
                genes.append(g)
                out.append(np.float32(acc[g]))
            out_off.append(len(genes))
    return np.array(out_off, dtype=np.uint64), np.array(genes, dtype=np.uint32), np.array(out, dtype=np.float32)


def make_case(label, cells, gene_of, n_genes=None):
    """cells: per cell a list of (col, val)."""
    indptr = np.cumsum([0] + [len(c) for c in cells]).astype(np.uint64)
    cols = np.array([e[0] for c in cells for e in c], dtype=np.uint32)
    vals = np.array([e[1] for c in cells for e in c], dtype=np.float32)
    gene_of = np.array(gene_of, dtype=np.uint32)
    if n_genes is None:
        n_genes = int(gene_of.max()) + 1 if len(gene_of) else 0
    return dict(label=label, indptr=indptr, cols=cols, vals=vals, gene_of=gene_of, n_genes=n_genes)


ORDER_VALS = [1.0, 2.0 ** -24, 2.0 ** -54, 2.0 ** -54, 2.0 ** -54, 2.0 ** -54]
ACC_VALS = [1.0, 2.0 ** -25, 2.0 ** -25, 2.0 ** -25]


def runs_case(n_runs, one_cell=True):
    """n_runs runs of one to three entries, in one cell or one run per cell; gene_of interleaves the genes."""
    n_txps = 3 * n_runs
    gene_of = [t % n_runs for t in range(n_txps)]
    ents = [[(t, 0.25 + (t % 7)) for t in range(n_txps) if t % n_runs == g and t // n_runs <= g % 3] for g in range(n_runs)]
    if one_cell:
        return make_case(f"{n_runs} runs in one cell", [sorted(e for run in ents for e in run)], gene_of)
    return make_case(f"{n_runs} cells of one run", ents, gene_of)


def named_cases():
    cs = [
        make_case("no cells", [], [0, 1, 2]),
        make_case("empty cells first, in the middle and last; a one-entry cell",
                  [[], [(0, 1.5), (2, 2.5)], [], [], [(1, 3.0)], []], [0, 1, 0]),
        make_case("gene_of not monotone, genes interleaved over the transcripts",
                  [[(t, 1.0 + t) for t in range(8)], [(1, 0.5), (4, 0.25), (6, 0.125), (7, 4.0)]], [2, 0, 1, 0, 2, 1, 0, 2]),
        make_case("gene ids with gaps: 0, n_genes - 1, and ids nobody has",
                  [[(0, 1.0), (1, 2.0), (2, 3.0)], [(2, 1.0)], [(0, 7.0)]], [0, 9, 0], n_genes=10),
        make_case("n_genes = 1", [[(0, 1.0), (1, 2.0)], [], [(2, 4.0)]], [0, 0, 0], n_genes=1),
        make_case("n_genes = 2^31 + 1 with the ids 0 and 2^31",
                  [[(0, 1.0), (1, 2.0), (2, 4.0)], [(1, 8.0)], [(0, 16.0), (3, 32.0)], [(1, 1.0), (3, 2.0)]],
                  [0, 2 ** 31, 0, 2 ** 31], n_genes=2 ** 31 + 1),
        make_case("the last entry of a cell and the first of the next in one gene",
                  [[(0, 1.0), (3, 2.0)], [(2, 4.0), (3, 8.0)], [(2, 16.0)]], [0, 0, 1, 1]),
        make_case("all entries of a cell in one gene", [[(t, 0.5 * (t + 1)) for t in range(7)]], [3] * 7),
        make_case("every entry a gene of its own", [[(t, 1.0 + t) for t in range(9)], [(8, 1.0), (0, 2.0)]], list(range(9))[::-1]),
        make_case("order inside a run: CSR order", [list(enumerate(ORDER_VALS))], [0] * 6),
        make_case("order inside a run: the same values backwards", [list(enumerate(ORDER_VALS[::-1]))], [0] * 6),
        make_case("an f64 accumulator", [list(enumerate(ACC_VALS))], [0] * 4),
        make_case("f32 denormals", [[(0, 2.0 ** -149), (1, 2.0 ** -149)], [(0, 2.0 ** -149)]], [0, 0]),
        make_case("+0.0 entries stay", [[(0, 0.0), (1, 0.0), (2, 1.0)], [(1, 0.0)]], [0, 0, 1]),
        make_case("f32 max twice", [[(0, F32_MAX), (1, F32_MAX), (2, F32_MAX)]], [0, 0, 1]),
    ]
    return cs


def random_case(seed=5, n_cells=8, per_cell=300, n_txps=40, n_genes=12):
    """Entries in no column order and with repeated columns: the rule takes the CSR as it is."""
    rng = np.random.default_rng(seed)
    gene_of = rng.integers(0, n_genes, size=n_txps)
    gene_of[:n_genes] = rng.permutation(n_genes)
    cells = [[(int(t), float(np.float32(rng.random() * 10.0 ** rng.integers(-3, 4)))) for t in rng.integers(0, n_txps, size=per_cell)]
             for _ in range(n_cells)]
    return make_case("random", cells, gene_of, n_genes=n_genes)


def edge_run_cases():
    return [runs_case(n) for n in (1, 63, 64, 65, 255, 256, 257)] + [runs_case(257, one_cell=False)]


def all_cases():
    return named_cases() + edge_run_cases() + [random_case()]


def same(got, want):
    """cell_off and genes equal, values bit for bit."""
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            and np.array_equal(np.asarray(got[2]).view(np.uint32), np.asarray(want[2]).view(np.uint32))
            and got[0].dtype == np.uint64 and got[1].dtype == np.uint32 and got[2].dtype == np.float32)


def call(L, fn, case, device=None, out=True, **over):
    """oem_cells_gene_counts (device given) or the hook (device None): (rc, message, result or None)."""
    a = dict(case)
    a.update(over)
    ptr = lambda x: None if x is None else x.ctypes.data   # noqa: E731
    n_cells = a.get("n_cells", 0 if a["indptr"] is None else len(a["indptr"]) - 1)
    n_txps = a.get("n_txps", 0 if a["gene_of"] is None else len(a["gene_of"]))
    h = C.c_void_p(1)
    args = [ptr(a["indptr"]), n_cells, ptr(a["cols"]), ptr(a["vals"]), ptr(a["gene_of"]), n_txps, a["n_genes"]]
    if device is not None:
        args.append(device)
    rc = getattr(L, fn)(*args, C.byref(h) if out else None)
    msg = L.oem_last_error().decode() if rc else ""
    if rc:
        assert h.value is None or not out
        return rc, msg, None
    return rc, msg, _take_cells_result(h, n_cells, L)[:3]


def test_the_value_cases_cannot_go_vacuous():
    """On this file's walk alone: CSR order and reversed order differ, and so do the f64 and the f32 accumulator."""
    by = {c["label"]: c for c in named_cases()}
    one, up = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
    fwd, bwd = by["order inside a run: CSR order"], by["order inside a run: the same values backwards"]
    assert walk(fwd["indptr"], fwd["cols"], fwd["vals"], fwd["gene_of"])[2].tolist() == [one]
    assert walk(bwd["indptr"], bwd["cols"], bwd["vals"], bwd["gene_of"])[2].tolist() == [up]
    assert walk(fwd["indptr"], fwd["cols"], fwd["vals"], fwd["gene_of"], reverse=True)[2].tolist() == [up]
    acc = by["an f64 accumulator"]
    assert walk(acc["indptr"], acc["cols"], acc["vals"], acc["gene_of"])[2].tolist() == [up]
    assert walk(acc["indptr"], acc["cols"], acc["vals"], acc["gene_of"], acc_type=np.float32)[2].tolist() == [one]
    den = by["f32 denormals"]
    assert walk(den["indptr"], den["cols"], den["vals"], den["gene_of"])[2].tolist() == [np.float32(2.0 ** -148), np.float32(2.0 ** -149)]
    z = by["+0.0 entries stay"]
    zo = walk(z["indptr"], z["cols"], z["vals"], z["gene_of"])
    assert zo[0].tolist() == [0, 2, 3] and zo[1].tolist() == [0, 1, 0] and zo[2].tolist() == [0.0, 1.0, 0.0]
    big = by["f32 max twice"]
    assert walk(big["indptr"], big["cols"], big["vals"], big["gene_of"])[2].tolist() == [np.inf, float(F32_MAX)]
    wide = by["n_genes = 2^31 + 1 with the ids 0 and 2^31"]
    wo = walk(wide["indptr"], wide["cols"], wide["vals"], wide["gene_of"])
    assert wo[0].tolist() == [0, 2, 3, 5, 6] and wo[1].tolist() == [0, 2 ** 31, 2 ** 31, 0, 2 ** 31, 2 ** 31]
    assert wo[2].tolist() == [5.0, 2.0, 8.0, 16.0, 32.0, 3.0]
    brk = by["the last entry of a cell and the first of the next in one gene"]
    assert walk(brk["indptr"], brk["cols"], brk["vals"], brk["gene_of"])[2].tolist() == [1.0, 2.0, 12.0, 16.0]


# ---------------------------------------------------------------------------------------------------------------------
# declared, exported, bound
# ---------------------------------------------------------------------------------------------------------------------
def test_declared_exported_and_bound():
    assert ENTRY in _b.header_symbols() and ENTRY in _lib.ABI_SYMBOLS
    assert HOOK in _b.TESTING_HOOKS and HOOK not in _b.header_symbols()
    exported = lambda p: {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", p], text=True).splitlines() if ln.strip()}  # noqa: E731
    prod, test = exported(_b.LIB_PATH), exported(_b.TESTING_LIB_PATH)
    assert ENTRY in prod and ENTRY in test and HOOK in test and HOOK not in prod
    assert hasattr(_lib.lib(), ENTRY) and hasattr(_lib.testing_lib(), HOOK)
    import oarfish_amd
    assert oarfish_amd.cells_gene_counts is cells_gene_counts and "cells_gene_counts" in oarfish_amd.__all__


# ---------------------------------------------------------------------------------------------------------------------
# the host walk: the testing library's hook, and the stand-alone program under sanitizers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", all_cases(), ids=lambda c: c["label"])
def test_the_host_walk_through_the_hook(case):
    rc, msg, got = call(_lib.testing_lib(), HOOK, case)
    assert rc == _lib.OEM_OK, msg
    assert same(got, walk(case["indptr"], case["cols"], case["vals"], case["gene_of"])), case["label"]


def test_the_hook_result_is_an_ordinary_cells_result():
    """infos zero-filled, no discard tables."""
    L = _lib.testing_lib()
    case = named_cases()[1]
    h = C.c_void_p()
    n_cells = len(case["indptr"]) - 1
    assert L.oem_test_cells_gene_counts_host(case["indptr"].ctypes.data, n_cells, case["cols"].ctypes.data, case["vals"].ctypes.data,
                                             case["gene_of"].ctypes.data, len(case["gene_of"]), case["n_genes"], C.byref(h)) == _lib.OEM_OK
    try:
        nc, ne = C.c_uint32(0), C.c_uint64(0)
        assert L.oem_cells_result_dims(h, C.byref(nc), C.byref(ne)) == _lib.OEM_OK and (nc.value, ne.value) == (n_cells, 2)
        infos = (_lib.RunInfoC * n_cells)()
        assert L.oem_cells_result_copy(h, None, None, None, C.addressof(infos)) == _lib.OEM_OK
        assert bytes(infos) == bytes(C.sizeof(infos))
        dts = (_lib.DiscardTableC * n_cells)()
        assert L.oem_cells_result_discard_tables(h, C.addressof(dts)) == _lib.OEM_ERR_STATE
    finally:
        L.oem_cells_result_destroy(h)


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-o", EXE, SRC])
    return EXE


def _request(case):
    lines = [f"G {len(case['indptr']) - 1} {len(case['cols'])} {len(case['gene_of'])}", " ".join(str(int(x)) for x in case["indptr"])]
    lines += [f"{int(c)} {int(b)}" for c, b in zip(case["cols"], case["vals"].view(np.uint32))]
    lines.append(" ".join(str(int(g)) for g in case["gene_of"]))
    return "\n".join(lines)


def test_the_host_walk_under_sanitizers(exe):
    cases = all_cases()
    r = subprocess.run([exe], input="\n".join(_request(c) for c in cases) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[-1] == "" and len(out) == len(cases) + 1
    for case, line in zip(cases, out):
        parts = [[int(x) for x in p.split()] for p in line.split("|")[1:]]
        assert line.startswith("ok") and len(parts) == 3, (case["label"], line)
        got = (np.cumsum([0] + parts[0]).astype(np.uint64), np.array(parts[1], dtype=np.uint32),
               np.array(parts[2], dtype=np.uint32).view(np.float32))
        assert same(got, walk(case["indptr"], case["cols"], case["vals"], case["gene_of"])), case["label"]


# ---------------------------------------------------------------------------------------------------------------------
# argument errors, before any device use
# ---------------------------------------------------------------------------------------------------------------------
GOOD = make_case("good", [[(0, 1.0), (9, 0.5)], [], [(4, 2.0)]], [0, 1, 2, 3, 4, 0, 1, 2, 3, 4], n_genes=5)
u64 = lambda *v: np.array(v, dtype=np.uint64)   # noqa: E731
u32 = lambda *v: np.array(v, dtype=np.uint32)   # noqa: E731

ARG_ERRORS = [
    ("cell_off NULL, n_cells 3", dict(indptr=None, n_cells=3), "cell_off is NULL and n_cells is not 0"),
    ("cell_off[0] != 0", dict(indptr=u64(1, 2, 2, 3)), "cell_off[0] must be 0"),
    ("cell_off decreasing", dict(indptr=u64(0, 2, 1, 3)), "cell_off must be non-decreasing (cell 1)"),
    ("col NULL with entries", dict(cols=None), "col or val is NULL"),
    ("val NULL with entries", dict(vals=None), "col or val is NULL"),
    ("gene_of NULL with entries", dict(gene_of=None, n_txps=10), "gene_of is NULL"),
    ("col == n_txps: the smallest entry is named", dict(cols=u32(0, 10, 11)), "col[1] = 10 is not below n_txps = 10"),
    ("col far above n_txps", dict(cols=u32(0, 9, 2 ** 32 - 1)), "col[2] = 4294967295 is not below n_txps = 10"),
    ("gene_of == n_genes: the smallest transcript is named", dict(gene_of=u32(0, 1, 2, 5, 4, 0, 1, 7, 3, 4)),
     "gene_of[3] = 5 is not below n_genes = 5"),
    ("n_genes = 0", dict(n_genes=0), "gene_of[0] = 0 is not below n_genes = 0"),
    # (the check of the cells' sizes reads cell_off alone: the entry arrays are never touched)
    ("a cell of 2^30 + 1 entries", dict(indptr=u64(0, 1, 2 ** 30 + 2, 2 ** 30 + 2)), "cell 1 has 1073741825 entries, more than 2^30"),
]


@pytest.mark.parametrize("name,over,text", ARG_ERRORS, ids=[e[0] for e in ARG_ERRORS])
@pytest.mark.parametrize("which", ["entry", "hook"])
def test_argument_errors_come_before_the_device(which, name, over, text):
    if which == "entry":
        rc, msg, _ = call(_lib.lib(), ENTRY, GOOD, device=0, **over)
        who = ENTRY
    else:
        rc, msg, _ = call(_lib.testing_lib(), HOOK, GOOD, **over)
        who = HOOK
    assert rc == _lib.OEM_ERR_ARG, (name, msg)
    assert msg.startswith(who + ": ") and text in msg, msg


def test_a_cell_of_exactly_2_30_entries_passes_the_size_check():
    """... and then fails on what comes next (col is NULL): the bound itself is legal."""
    rc, msg, _ = call(_lib.lib(), ENTRY, GOOD, device=0, indptr=u64(0, 2 ** 30), cols=None)
    assert rc == _lib.OEM_ERR_ARG and "col or val is NULL" in msg


def test_null_out_is_an_argument_error():
    for L, fn, dev in ((_lib.lib(), ENTRY, 0), (_lib.testing_lib(), HOOK, None)):
        rc, msg, _ = call(L, fn, GOOD, device=dev, out=False)
        assert rc == _lib.OEM_ERR_ARG and "out is NULL" in msg


def test_fails_loudly_without_a_device():
    """A valid call -- an empty one too -- says OEM_ERR_NO_DEVICE where there is none: there is no host fallback."""
    for case in (GOOD, named_cases()[0]):
        rc, msg, got = call(_lib.lib(), ENTRY, case, device=0)
        if _lib.device_count() > 0:
            assert rc == _lib.OEM_OK and same(got, walk(case["indptr"], case["cols"], case["vals"], case["gene_of"]))
        else:
            assert rc == _lib.OEM_ERR_NO_DEVICE and got is None, msg


def test_python_wrapper_checks_its_own_arguments():
    with pytest.raises(ValueError):
        cells_gene_counts([], [], [], [0])
    with pytest.raises(ValueError):
        cells_gene_counts([0, 2], [1], [1.0], [0, 0])
    with pytest.raises(ValueError):
        cells_gene_counts([0, 1], [1], [1.0, 2.0], [0, 0])
    with pytest.raises(ValueError):
        cells_gene_counts([0, 1], [1], [1.0], [[0, 0]])
    with pytest.raises(ValueError):
        cells_gene_counts([0, 1], [1], [1.0], [0, -1])
    with pytest.raises(ValueError):
        cells_gene_counts([0, 1], [1], [1.0], [0.0, 1.0])
    with pytest.raises(ValueError):
        cells_gene_counts([0, 1], [1], [1.0], [0, 0], n_genes=2 ** 32)
    with pytest.raises(_lib.OemError) as ei:   # n_genes=None is max(gene_of) + 1; a smaller one is the library's error
        cells_gene_counts([0, 1], [1], [1.0], [0, 3], n_genes=3)
    assert ei.value.code == _lib.OEM_ERR_ARG and "gene_of[1] = 3 is not below n_genes = 3" in str(ei.value)
