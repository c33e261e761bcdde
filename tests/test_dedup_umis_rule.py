"""CPU tests of the UMI rule (gene_of, correct) -- oem_dedup_umis_rule, oem_em_run_cells_records_umis_rule_sparse: declared,
exported by both libraries and bound; the host walk of the rule (oarfish_amd/csrc/oem_collate.h, dedup_umis_rule_host)
against a walk written here; the same walk in a stand-alone program under the address and undefined-behaviour sanitizers;
the rule's argument errors before any device use; the Python wrappers' own checks; the synthetic UMI errors.

The walk here knows nothing of the C++ one: per cell a dict from (gene, UMI bytes) to the groups of the class, all pairs
of classes for the neighbours, parents from the original counts, roots by following them.  It also counts what a case
exercises (corrected classes, the longest chain, ties), so that the random cases can be held to exercising the rule.
tests/test_dedup_umis_rule_gpu.py holds the device to the host walk on the same cases."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth
from oarfish_amd import build as _b
from oarfish_amd.em import UmiRuleC, gather_names
from tests.test_dedup_umis import FILTERS, UNMAPPED, _input, host_walk, make_case, pack, umi_cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "dedup_umis_rule_main.cpp")
EXE = os.path.join(HERE, "native", "dedup_umis_rule_main")
HDR = os.path.join(ROOT, "oarfish_amd", "csrc", "oem_collate.h")
DEDUP = "oem_dedup_umis_rule"
ONE_CALL = "oem_em_run_cells_records_umis_rule_sparse"
HOOK = "oem_test_dedup_umis_rule_host"
N_TXPS = 8
GENES = list(range(N_TXPS))                 # transcript t is gene t
PAIRS = [t // 2 for t in range(N_TXPS)]     # transcripts 2 g and 2 g + 1 are gene g
COMBOS = [(False, False), (True, False), (False, True), (True, True)]   # (with gene_of, correct)


# ---------------------------------------------------------------------------------------------------------------------
# the walk and the cases
# ---------------------------------------------------------------------------------------------------------------------
def neighbours(a, b):
    return len(a) == len(b) and sum(x != y for x, y in zip(a, b)) == 1


def restate_rule(case, gene_of, correct):
    """(dup, survivor, cell_dups, cell_corrected) as lists, and what the case exercised, from the rule as the issue states
    it.  A bad head ref_id gives ("badref", the smallest such input index)."""
    umis, flags, order, goff, cgo, ref_id = (case[k] for k in ("umis", "flags", "order", "group_off", "cell_group_off", "ref_id"))
    ng, nc = len(goff) - 1, len(cgo) - 1
    dup, survivor, cell_dups, cell_corrected = [0] * ng, list(range(ng)), [0] * nc, [0] * nc
    stats = dict(corrected_classes=0, depth=0, ties=0)

    def takes_part(g):
        if goff[g + 1] == goff[g]:
            return False
        head = order[goff[g]]
        return bool(umis[head]) and not (flags is not None and flags[head] & UNMAPPED)

    if gene_of is not None:
        bad = [order[goff[g]] for g in range(ng) if takes_part(g) and ref_id[order[goff[g]]] >= len(gene_of)]
        if bad:
            return "badref", min(bad)
    for c in range(nc):
        classes = {}                                   # (gene, UMI) -> its groups, ascending
        for g in range(cgo[c], cgo[c + 1]):
            if takes_part(g):
                head = order[goff[g]]
                classes.setdefault((0 if gene_of is None else gene_of[ref_id[head]], umis[head]), []).append(g)
        parent = {}
        if correct:
            for u, gu in classes.items():
                cands = [v for v, gv in classes.items() if v[0] == u[0] and neighbours(u[1], v[1]) and len(gv) > len(gu)]
                if cands:
                    most = max(len(classes[v]) for v in cands)
                    best = sorted(v[1] for v in cands if len(classes[v]) == most)
                    stats["ties"] += len(best) > 1
                    parent[u] = (u[0], best[0])
        stats["corrected_classes"] += len(parent)
        molecules = {}
        for u in classes:
            r, depth = u, 0
            while r in parent:
                r, depth = parent[r], depth + 1
            stats["depth"] = max(stats["depth"], depth)
            molecules.setdefault(r, []).extend(classes[u])
        for u, groups in classes.items():
            if u in parent:
                cell_corrected[c] += len(groups)
        for groups in molecules.values():
            first = min(groups)
            for g in groups:
                if g != first:
                    dup[g], survivor[g] = 1, first
                    cell_dups[c] += 1
    return (dup, survivor, cell_dups, cell_corrected), stats


def make_rule_case(cells, seed=0, with_flags=True):
    """tests/test_dedup_umis.py's make_case with a transcript per record: a record is ``umi``, ``(umi, flags)`` or ``(umi,
    flags, ref_id)``; ``ref_id`` defaults to 0.  The records' genes travel through ``ref_id`` and the rule's ``gene_of``."""
    full = [(r if isinstance(r, tuple) else (r, 0)) + (0,) * (3 - len(r if isinstance(r, tuple) else (r, 0)))
            for cell in cells for group in cell for r in group]
    plain = [[[(r if isinstance(r, tuple) else (r, 0))[:2] for r in group] for group in cell] for cell in cells]
    case = make_case(plain, seed=seed, with_flags=with_flags)
    ref_id = [0] * len(full)
    for k, (_, _, t) in enumerate(full):
        ref_id[case["order"][k]] = t
    return dict(case, ref_id=ref_id)


def with_refs(case, n_txps=N_TXPS):
    """A case of tests/test_dedup_umis.py with transcripts dealt round the records."""
    return dict(case, ref_id=[(5 * i + 3) % n_txps for i in range(len(case["umis"]))])


def reads(umi, n=1, txp=0, flags=0):
    """n reads (groups of one record) with one UMI and transcript."""
    return [[(umi, flags, txp)] for _ in range(n)]


def rule_cases():
    """name -> case.  Every case runs under all four (gene_of, correct) with GENES, and under PAIRS."""
    cases = {}
    a, b, c = b"AAAAAAAAAAAA", b"AAAAAAAAAAAT", b"AAAAAAAAAATT"          # c is b's neighbour, not a's
    cases["chain_3_2_1"] = make_rule_case([reads(c) + reads(b, 2) + reads(a, 3)], seed=1)
    cases["chain_in_input_order"] = make_rule_case([reads(c) + reads(b, 2) + reads(a, 3)], seed=None)
    cases["equal_counts_do_not_merge"] = make_rule_case([reads(b"ACGT") + reads(b"ACGA") + reads(b"TTTT", 2) + reads(b"TTTA", 2)], seed=2)
    cases["a_tie_goes_to_the_smaller_bytes"] = make_rule_case([reads(b"AAAG", 2) + reads(b"AAAC", 2) + reads(b"AAAT")], seed=3)
    cases["more_groups_beat_smaller_bytes"] = make_rule_case([reads(b"AAAC", 2) + reads(b"TAAA", 3) + reads(b"AAAA")], seed=4)
    base = b"ACGTACGTTGCATGCAA"                                             # 17 bytes: two whole keys and a byte
    for length in (1, 2, 8, 9, 16, 17):
        u = base[:length]
        spots = sorted({0, length - 1, length // 2, min(7, length - 1), min(8, length - 1)})
        cell = reads(u, 3)
        for k, at in enumerate(spots):   # one error per position: at byte 0, the last, 7 and 8, and the middle
            cell += reads(u[:at] + b"N" + u[at + 1:], 1 + k % 2)
        cases[f"one_mismatch_at_every_edge_of_{length}_bytes"] = make_rule_case([cell], seed=10 + length)
    cases["acg_and_acgt_are_never_neighbours"] = make_rule_case([reads(b"ACG") + reads(b"ACGT", 2) + reads(b"AC", 3) + reads(b"A", 4)], seed=5)
    cases["bytes_outside_acgt"] = make_rule_case([reads(b"ACGN") + reads(b"ACGT", 2) + reads(b"acgt") + reads(b"acgT", 3)
                                                  + reads(b"AC\xffT") + reads(b"AC\xfeT", 2) + reads(b"\x01\x01", 2) + reads(b"\x01\x02")], seed=6)
    x = b"AACCGGTTAACC"
    cases["one_umi_in_two_genes_of_a_cell"] = make_rule_case([reads(x, 2, txp=1) + reads(x, 2, txp=4) + reads(x, 1, txp=1)], seed=7)
    y = x[:-1] + b"G"
    cases["a_neighbour_in_another_gene_or_cell"] = make_rule_case([reads(x, 3, txp=2) + reads(y, 1, txp=5), reads(y, 1, txp=2)], seed=8)
    cases["non_participants"] = make_rule_case(
        [reads(x, 2) + [[(b"", 0, 0)], [(y, UNMAPPED, 0)], [(y, UNMAPPED, 0), (y, 0, 0)], []] + reads(y, 1) + [[(y, UNMAPPED, 0)]]], seed=9)
    cases["non_participants_without_flags"] = make_rule_case([reads(x, 2) + [[(y, UNMAPPED, 0)], [(b"", 0, 0)]]], seed=9, with_flags=False)
    # the corrected class's only group comes first in the cell: it survives, and its parent's groups are its duplicates
    cases["the_survivor_is_a_corrected_group"] = make_rule_case([reads(y, 1) + reads(x, 2)], seed=None)
    cases["two_transcripts_of_one_gene"] = make_rule_case([reads(x, 2, txp=2) + reads(x, 1, txp=3) + reads(y, 1, txp=3) + reads(x, 1, txp=4)],
                                                          seed=11)
    cases["non_head_record_with_another_umi_and_gene"] = make_rule_case(
        [[[(x, 0, 1), (y, 0, 6)], [(y, 0, 1)], [(x, 0, 1)], [(y, 0, 6), (x, 0, 1)]]], seed=12)
    cases["three_cells_and_an_empty_one"] = make_rule_case(
        [reads(x, 2) + reads(y), [], reads(y, 2, txp=3) + reads(x, 1, txp=3) + reads(x, 1, txp=6), reads(x)], seed=13)
    return cases


def random_case(seed, n_cells=8, n_reads=300, n_genes=6, n_molecules=6, umi_len=5, p_error=0.15, p_empty=0.03):
    """Cells of reads drawn from n_genes x n_molecules molecules with log-normal weights; the per-base substitution at
    p_error is applied to a read's UMI twice over, so that errors of errors (chains) occur; gene g is transcripts 2 g and
    2 g + 1.  Returns (case, gene_of)."""
    rng = np.random.default_rng([seed, 0xC0DE])
    nuc = np.frombuffer(b"ACGT", dtype=np.uint8)
    cells = []
    for _ in range(n_cells):
        true = nuc[rng.integers(0, 4, size=(n_genes * n_molecules, umi_len))]
        w = rng.lognormal(0.0, 1.0, size=len(true))
        pick = rng.choice(len(true), size=n_reads, p=w / w.sum())
        cell = []
        for m in pick:
            u = true[m].copy()
            for _pass in range(2):
                hit = rng.random(umi_len) < p_error
                u[hit] = nuc[rng.integers(0, 4, size=int(hit.sum()))]
            umi = b"" if rng.random() < p_empty else u.tobytes()
            cell.append([(umi, 0, 2 * int(m // n_molecules) + int(rng.integers(0, 2)))])
        cells.append(cell)
    return make_rule_case(cells, seed=seed), [t // 2 for t in range(2 * n_genes)]


def test_the_walk_itself():
    cases = rule_cases()
    got, stats = restate_rule(cases["chain_in_input_order"], GENES, True)      # groups: c, b, b, a, a, a
    assert got == ([0, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0], [5], [3]) and stats == dict(corrected_classes=2, depth=2, ties=0)
    assert restate_rule(cases["chain_in_input_order"], GENES, False)[0] == ([0, 0, 1, 0, 1, 1], [0, 1, 1, 3, 3, 3], [3], [0])
    for name in ("equal_counts_do_not_merge", "acg_and_acgt_are_never_neighbours"):
        assert restate_rule(cases[name], GENES, True)[0] == restate_rule(cases[name], GENES, False)[0], name
        assert restate_rule(cases[name], GENES, True)[1]["corrected_classes"] == 0, name

    def molecule_of(case, umi, correct=True, gene_of=GENES):
        """The UMIs of the heads of the molecule that the (first) read with `umi` belongs to."""
        (dup, survivor, _, _), _ = restate_rule(case, gene_of, correct)
        heads = [case["umis"][case["order"][p]] for p in case["group_off"][:-1]]
        s = survivor[heads.index(umi)]
        return sorted({heads[g] for g in range(len(heads)) if survivor[g] == s})

    assert molecule_of(cases["a_tie_goes_to_the_smaller_bytes"], b"AAAT") == [b"AAAC", b"AAAT"]
    assert restate_rule(cases["a_tie_goes_to_the_smaller_bytes"], GENES, True)[1]["ties"] == 1
    assert molecule_of(cases["more_groups_beat_smaller_bytes"], b"AAAA") == [b"AAAA", b"TAAA"]
    for length in (1, 2, 8, 9, 16, 17):
        (dup, _, cell_dups, cell_corrected), stats = restate_rule(cases[f"one_mismatch_at_every_edge_of_{length}_bytes"], GENES, True)
        n_spots = len({0, length - 1, length // 2, min(7, length - 1), min(8, length - 1)})
        assert stats["corrected_classes"] == n_spots and cell_dups == [len(dup) - 1] and cell_corrected == [len(dup) - 3], length
    got, stats = restate_rule(cases["bytes_outside_acgt"], GENES, True)
    assert stats["corrected_classes"] == 4 and got[3] == [4]
    two = cases["one_umi_in_two_genes_of_a_cell"]
    assert restate_rule(two, GENES, False)[0][2] == [3] and restate_rule(two, None, False)[0][2] == [4]
    other = cases["a_neighbour_in_another_gene_or_cell"]
    assert restate_rule(other, GENES, True)[0][2:] == ([2, 0], [0, 0]) and restate_rule(other, None, True)[0][2:] == ([3, 0], [1, 0])
    got, stats = restate_rule(cases["non_participants"], GENES, True)
    assert got[2:] == ([2], [1]) and stats["corrected_classes"] == 1
    assert restate_rule(cases["non_participants_without_flags"], GENES, True)[0][2:] == ([2], [1])
    assert restate_rule(cases["the_survivor_is_a_corrected_group"], GENES, True)[0] == ([0, 1, 1], [0, 0, 0], [2], [1])
    pair = cases["two_transcripts_of_one_gene"]
    assert restate_rule(pair, GENES, True)[0][2:] == ([1], [0]) and restate_rule(pair, PAIRS, True)[0][2:] == ([3], [1])
    assert restate_rule(cases["non_head_record_with_another_umi_and_gene"], GENES, False)[0][:2] == ([0, 0, 1, 0], [0, 1, 0, 3])
    # a bad ref_id counts only at the head of a read that takes part; the smallest input index is named
    bad = make_rule_case([[[(x, 0, 9)] for x in (b"AC", b"AC")] + [[(b"AC", UNMAPPED, 9)], [(b"", 0, 9)], [(b"G", 0, 1), (b"G", 0, 9)]]], seed=None)
    assert restate_rule(bad, GENES, False) == ("badref", 0) and restate_rule(bad, None, True)[0][0] == [0, 1, 0, 0, 0]
    bad["ref_id"][0] = 1
    assert restate_rule(bad, GENES, False) == ("badref", 1)
    bad["ref_id"][1] = 1
    assert restate_rule(bad, GENES, False)[0][0] == [0, 1, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------
# declared, exported, bound
# ---------------------------------------------------------------------------------------------------------------------
def _declaration(name):
    src = open(os.path.join(ROOT, "include", "oarfish_em.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
    assert m, "include/oarfish_em.h does not declare " + name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,n_args,second,last", [(DEDUP, 17, "const uint8_t *umis", "uint64_t *out_cell_corrected"),
                                                     (ONE_CALL, 31, "const oem_filters *filters", "oem_cells_result **out")])
def test_declared_exported_by_both_libraries_and_bound(name, n_args, second, last):
    args = _declaration(name)
    assert len(args) == n_args and args[0] == "const oem_umi_rule *rule" and args[1] == second and args[-1] == last
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
    assert HOOK in _b.TESTING_HOOKS
    out = subprocess.check_output(["nm", "-D", "--defined-only", _b.LIB_PATH], text=True)
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip()) == sorted(_b.header_symbols())
    assert C.sizeof(UmiRuleC) == 16


# ---------------------------------------------------------------------------------------------------------------------
# the host walk: the testing library's hook, and the stand-alone program under sanitizers
# ---------------------------------------------------------------------------------------------------------------------
def call_rule(L, fn, case, gene_of, correct, device=None, with_ref_id=True, rule=True, with_corrected=True):
    """oem_dedup_umis_rule (device = 0) or the hook (device = None): (rc, message, dup, survivor, cell_dups, cell_corrected)."""
    blob, off = pack(case["umis"])
    n = len(case["umis"])
    order = np.array(case["order"], dtype=np.uint32)
    goff, cgo = np.array(case["group_off"], dtype=np.uint64), np.array(case["cell_group_off"], dtype=np.uint64)
    flags = None if case["flags"] is None else np.array(case["flags"], dtype=np.uint32)
    ref_id = np.array(case["ref_id"] or [0], dtype=np.uint32)
    gene = None if gene_of is None else np.array(gene_of, dtype=np.uint32)
    r = UmiRuleC(None if gene is None else gene.ctypes.data, 0 if gene is None else len(gene), int(correct))
    ng, nc = len(goff) - 1, len(cgo) - 1
    dup = np.full(max(ng, 1), 0xEE, dtype=np.uint8)
    survivor = np.full(max(ng, 1), 2 ** 64 - 1, dtype=np.uint64)
    cell_dups = np.full(max(nc, 1), 2 ** 64 - 1, dtype=np.uint64)
    cell_corrected = np.full(max(nc, 1), 2 ** 64 - 1, dtype=np.uint64)
    if not len(blob):
        blob = np.zeros(1, dtype=np.uint8)
    head = [C.addressof(r) if rule else None, blob.ctypes.data, off.ctypes.data, None if flags is None or not len(flags) else flags.ctypes.data,
            ref_id.ctypes.data if with_ref_id else None, n, order.ctypes.data if len(order) else None, len(order), goff.ctypes.data, ng,
            cgo.ctypes.data, nc]
    rc = getattr(L, fn)(*head, *([] if device is None else [device]), dup.ctypes.data, survivor.ctypes.data, cell_dups.ctypes.data,
                        cell_corrected.ctypes.data if with_corrected else None)
    return rc, (L.oem_last_error() or b"").decode(), dup[:ng].tolist(), survivor[:ng].tolist(), cell_dups[:nc].tolist(), \
        cell_corrected[:nc].tolist()


def rule_host_walk(case, gene_of, correct):
    rc, msg, *got = call_rule(_lib.testing_lib(), HOOK, case, gene_of, correct)
    assert rc == _lib.OEM_OK, msg
    return tuple(got)


def all_cases():
    """(label, case, gene_of, correct) of everything the host walk and the device are compared on."""
    out = []
    for name, case in rule_cases().items():
        out += [(f"{name}, genes {g}, correct {c}", case, GENES if g else None, c) for g, c in COMBOS]
        out += [(f"{name}, transcript pairs", case, PAIRS, True)]
    for name, case in umi_cases().items():
        out += [(f"{name} (exact-rule case), genes {g}, correct {c}", with_refs(case), GENES if g else None, c) for g, c in COMBOS]
    return out


def test_the_host_walk_equals_the_walk_here():
    for label, case, gene_of, correct in all_cases():
        assert rule_host_walk(case, gene_of, correct) == restate_rule(case, gene_of, correct)[0], label


def test_the_default_rule_is_the_exact_rule():
    L = _lib.testing_lib()
    for name, case in umi_cases().items():
        want = host_walk(case)
        nc = len(case["cell_group_off"]) - 1
        assert rule_host_walk(with_refs(case), None, False) == (*want, [0] * nc), name
        for kw in (dict(rule=False), dict(with_ref_id=False), dict(with_corrected=False)):   # a NULL rule, no ref_id, no cell_corrected
            rc, msg, *got = call_rule(L, HOOK, with_refs(case), None, False, **kw)
            assert rc == _lib.OEM_OK and tuple(got[:3]) == want, (name, kw, msg)


@pytest.mark.parametrize("seed", range(5))
def test_the_host_walk_on_random_cells_that_exercise_the_rule(seed):
    case, gene_of = random_case(seed)
    want, stats = restate_rule(case, gene_of, True)
    # asserted on the walk here, not on the code under test: the input must exercise the rule
    assert stats["corrected_classes"] >= 100 and stats["depth"] >= 2 and stats["ties"] >= 1, stats
    assert want != restate_rule(case, None, True)[0]
    assert sum(1 for u in case["umis"] if not u) > 0
    assert rule_host_walk(case, gene_of, True) == want
    for g, c in COMBOS[:3]:
        assert rule_host_walk(case, gene_of if g else None, c) == restate_rule(case, gene_of if g else None, c)[0], (g, c)


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-o", EXE, SRC])
    return EXE


def _request(case, gene_of, correct):
    n, flags = len(case["umis"]), case["flags"]
    lines = [f"R {n} {len(case['order'])} {len(case['group_off']) - 1} {len(case['cell_group_off']) - 1} {int(flags is not None)} "
             f"{0 if gene_of is None else len(gene_of)} {int(correct)}"]
    lines += [f"{u.hex() or '-'} {0 if flags is None else flags[i]} {case['ref_id'][i]}" for i, u in enumerate(case["umis"])]
    lines += [" ".join(str(v) for v in case[k]) for k in ("order", "group_off", "cell_group_off")]
    lines += [" ".join(str(v) for v in (gene_of or []))]
    return "\n".join(lines) + "\n"


def _walk(exe, requests):
    r = subprocess.run([exe], input="".join(requests), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[-1] == "" and len(out) == len(requests) + 1
    return out[:-1]


def test_the_host_walk_under_sanitizers(exe):
    cases = all_cases()
    for seed in (0, 3):
        case, gene_of = random_case(seed)
        cases += [(f"random {seed}, genes {g}, correct {c}", case, gene_of if g else None, c) for g, c in COMBOS]
    for (label, case, gene_of, correct), line in zip(cases, _walk(exe, [_request(c, g, k) for _, c, g, k in cases])):
        parts = [[int(x) for x in p.split()] for p in line.split("|")[1:]]
        assert line.startswith("ok") and len(parts) == 4, (label, line)
        assert tuple(parts) == restate_rule(case, gene_of, correct)[0], label


BAD_REF = [[[(x, 0, 9)] for x in (b"AC", b"AC")] + [[(b"AC", UNMAPPED, 9)], [(b"", 0, 9)], [(b"G", 0, 1), (b"G", 0, 9)]]]


def test_a_bad_ref_id_at_a_head_that_takes_part(exe):
    L = _lib.testing_lib()
    bad = make_rule_case(BAD_REF, seed=None)
    rc, msg, *_ = call_rule(L, HOOK, bad, GENES, True)
    assert rc == _lib.OEM_ERR_ARG and "record 0: ref_id 9 is not below n_txps = 8" in msg, msg
    bad["ref_id"][0] = 1
    rc, msg, *_ = call_rule(L, HOOK, bad, GENES, False)
    assert rc == _lib.OEM_ERR_ARG and "record 1: ref_id 9 is not below n_txps = 8" in msg, msg
    assert _walk(exe, [_request(bad, GENES, False)]) == ["badref 1"]
    bad["ref_id"][1] = 1      # what is left: an unmapped head, the head of an empty UMI, a record that is no head
    assert rule_host_walk(bad, GENES, True) == restate_rule(bad, GENES, True)[0]
    assert rule_host_walk(bad, None, True) == restate_rule(bad, None, True)[0]     # without gene_of no ref_id is read
    zero = make_rule_case([[[b"AC"], [b"A\x00C"], [b"AC"]], [[b"\x00"]]], seed=None)
    rc, msg, *_ = call_rule(L, HOOK, zero, GENES, True)
    assert rc == _lib.OEM_ERR_ARG and "the UMI of record 1 contains a 0 byte" in msg
    assert _walk(exe, [_request(zero, GENES, True)]) == ["bad 1"]


# ---------------------------------------------------------------------------------------------------------------------
# argument errors before any device use, and the wrappers
# ---------------------------------------------------------------------------------------------------------------------
def test_rule_argument_errors_come_before_any_device_use():
    case = make_rule_case([reads(b"AC", 2) + reads(b"AG")], seed=None)
    gene = np.array(GENES, dtype=np.uint32)
    for L, fn, device in ((_lib.lib(), DEDUP, 0), (_lib.testing_lib(), DEDUP, 0), (_lib.testing_lib(), HOOK, None)):
        rc, msg, *_ = call_rule(L, fn, case, GENES, 2, device=device)
        assert rc == _lib.OEM_ERR_ARG and fn in msg and "correct = 2" in msg, msg
        rc, msg, *_ = call_rule(L, fn, case, GENES, True, device=device, with_ref_id=False)
        assert rc == _lib.OEM_ERR_ARG and fn in msg and "ref_id is NULL" in msg, msg
        blob, off = pack(case["umis"])
        r = UmiRuleC(gene.ctypes.data, 0, 1)
        out = [np.zeros(8, dtype=np.uint64) for _ in range(4)]
        order, goff, cgo = (np.array(case[k], dtype=t) for k, t in (("order", np.uint32), ("group_off", np.uint64), ("cell_group_off", np.uint64)))
        ref_id = np.zeros(3, dtype=np.uint32)
        rc = getattr(L, fn)(C.addressof(r), blob.ctypes.data, off.ctypes.data, None, ref_id.ctypes.data, 3, order.ctypes.data, 3, goff.ctypes.data,
                            3, cgo.ctypes.data, 1, *([] if device is None else [device]), *(o.ctypes.data for o in out))
        assert rc == _lib.OEM_ERR_ARG and b"n_txps is 0" in L.oem_last_error()
    # the exact call's own errors come from the same checks, under the new name
    rc, msg, *_ = call_rule(_lib.lib(), DEDUP, dict(case, group_off=[0, 1, 2, 4]), None, False, device=0)
    assert rc == _lib.OEM_ERR_ARG and DEDUP in msg and "group_off ends at 4, not at n_positions = 3" in msg


def _one_call(L, rule, a, n_txps=40, n=5):
    res = C.c_void_p(1)
    ptr = lambda x: None if x is None else x.ctypes.data   # noqa: E731
    rc = getattr(L, ONE_CALL)(None if rule is None else C.addressof(rule), C.addressof(a["F"]), ptr(a["tl"]), n_txps, ptr(a["rec"]), n,
                              ptr(a["bc_blob"]), ptr(a["bc_off"]), ptr(a["blob"]), ptr(a["off"]), ptr(a["sec"]), ptr(a["um_blob"]),
                              ptr(a["um_off"]), 0, 100, -1, 2.0, 0, 100, 1e-3, None, None, None, None, None, None, None, None, None, None,
                              C.byref(res))
    return rc, res, L.oem_last_error() or b""


def test_one_call_rule_argument_errors_come_before_any_device_use():
    L = _lib.lib()
    a = _input()
    gene = np.arange(40, dtype=np.uint32)
    for rule, word in ((UmiRuleC(None, 0, 2), b"correct = 2"), (UmiRuleC(gene.ctypes.data, 0, 0), b"n_txps is 0"),
                       (UmiRuleC(gene.ctypes.data, 39, 1), b"rule->n_txps = 39 is not n_txps = 40")):
        rc, res, msg = _one_call(L, rule, a)
        assert rc == _lib.OEM_ERR_ARG and not res.value and word in msg and ONE_CALL.encode() in msg, msg
    rc, res, msg = _one_call(L, UmiRuleC(gene.ctypes.data, 40, 1), dict(a, um_off=None))      # ... behind the umis call's own
    assert rc == _lib.OEM_ERR_ARG and b"umi_off is NULL" in msg and ONE_CALL.encode() in msg
    for rule in (None, UmiRuleC(None, 0, 0), UmiRuleC(gene.ctypes.data, 40, 1)):
        rc, res, msg = _one_call(L, rule, a)
        if _lib.device_count() > 0:
            assert rc == _lib.OEM_OK and res.value, msg
            L.oem_cells_result_destroy(res)
        else:
            assert rc == _lib.OEM_ERR_NO_DEVICE and not res.value, (rc, msg)


def test_the_wrappers_check_their_own_arguments():
    a = _input()
    names, barcodes, umis = (a["blob"], a["off"]), (a["bc_blob"], a["bc_off"]), (a["um_blob"], a["um_off"])
    run = lambda **kw: oarfish_amd.em_cells_records_sparse(FILTERS, a["tl"], a["rec"], None, None, names=names, barcodes=barcodes, **kw)   # noqa: E731
    for collate in ("host", "device"):
        with pytest.raises(ValueError, match="go with umis"):
            run(gene_of=np.arange(40), collate=collate)
        with pytest.raises(ValueError, match="go with umis"):
            run(umi_correct=True, collate=collate)
    with pytest.raises(ValueError, match="gene_of needs ref_id"):
        oarfish_amd.dedup_umis_rule(umis, [0, 1], [0, 1, 2], [0, 2], gene_of=[0, 1])
    with pytest.raises(ValueError, match="ref_id must have one entry per record"):
        oarfish_amd.dedup_umis_rule(umis, [0, 1], [0, 1, 2], [0, 2], ref_id=[0, 1], gene_of=[0, 1])
    with pytest.raises(ValueError, match="flags must have one entry per record"):
        oarfish_amd.dedup_umis_rule(umis, [0, 1], [0, 1, 2], [0, 2], flags=np.zeros(4, dtype=np.uint32))
    assert {"dedup_umis_rule", "add_umi_errors", "gene_of_txps"} <= set(oarfish_amd.__all__)
    if _lib.device_count() == 0:
        with pytest.raises(_lib.OemError) as e:
            oarfish_amd.dedup_umis_rule([b"AC", b"AG"], [0, 1], [0, 1, 2], [0, 2], ref_id=[0, 1], gene_of=[0, 0], correct=True)
        assert e.value.code == _lib.OEM_ERR_NO_DEVICE
        with pytest.raises(oarfish_amd.OemError) as e:
            run(umis=umis, gene_of=np.arange(40), umi_correct=True, collate="device")
        assert e.value.code == _lib.OEM_ERR_NO_DEVICE


# ---------------------------------------------------------------------------------------------------------------------
# the synthetic errors and genes
# ---------------------------------------------------------------------------------------------------------------------
def _strings(pair):
    raw, off = np.asarray(pair[0]).tobytes(), np.asarray(pair[1]).astype(np.int64)
    return [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def test_add_umi_errors_and_gene_of_txps():
    rng = np.random.default_rng(4)
    n_reads = 600
    read_umi = [bytes(rng.choice(list(b"ACGT"), size=12).astype(np.uint8)) for _ in range(n_reads)]
    read_umi[5] = read_umi[17] = b""
    read_of = rng.integers(0, n_reads, size=2000)
    names, barcodes = pack([b"read%d" % (r // 2) for r in read_of]), pack([b"AC" if r % 2 else b"GT" for r in read_of])
    umis = pack([read_umi[r] for r in read_of])
    before = _strings(umis)
    out = synth.add_umi_errors(umis, 0.25, seed=8, names=names, barcodes=barcodes)
    assert _strings(umis) == before                                            # the input is left alone
    after = _strings(out)
    assert np.array_equal(out[1], umis[1]) and out[1].dtype == np.uint64
    per_read = {}
    for r, u, v in zip(read_of, before, after):
        assert len(u) == len(v) and sum(x != y for x, y in zip(u, v)) <= 1 and set(v) <= set(b"ACGT")
        assert per_read.setdefault(int(r), v) == v                            # the same on all records of a read
    hit = sum(1 for r, v in per_read.items() if v != read_umi[r])
    assert 0.15 * len(per_read) < hit < 0.35 * len(per_read)
    # a pure function, of the read and the seed and not of the records' order
    assert _strings(synth.add_umi_errors(umis, 0.25, seed=8, names=names, barcodes=barcodes)) == after
    assert _strings(synth.add_umi_errors(umis, 0.25, seed=9, names=names, barcodes=barcodes)) != after
    perm = rng.permutation(2000)
    g = gather_names
    assert _strings(synth.add_umi_errors(g(umis, perm), 0.25, seed=8, names=g(names, perm), barcodes=g(barcodes, perm))) == [after[i] for i in perm]
    assert _strings(synth.add_umi_errors(umis, 0.0, names=names, barcodes=barcodes)) == before
    assert sum(x != y for x, y in zip(_strings(synth.add_umi_errors(umis, 1.0)), before)) == sum(1 for u in before if u)
    with pytest.raises(ValueError):
        synth.add_umi_errors(umis, 1.5)
    gene_of = synth.gene_of_txps(1000)
    assert gene_of.dtype == np.uint32 and len(gene_of) == 1000 and gene_of[0] == 0 and (np.diff(gene_of.astype(np.int64)) >= 0).all()
    assert set(np.diff(gene_of.astype(np.int64)).tolist()) == {0, 1} and 150 < int(gene_of[-1]) < 400
    assert np.array_equal(gene_of, synth.gene_of_txps(1000)) and not np.array_equal(gene_of, synth.gene_of_txps(1000, seed=1))
