"""GPU tests of barcode correction against a whitelist.  oem_correct_barcodes is held to the host walk of
oem_barcode_correct.h (the testing library's oem_test_correct_barcodes_host, itself held to the walk of
tests/test_correct_barcodes.py) in all outputs: on every CPU case and both random cases, from both libraries, at the table,
wavefront and launch edges, and with hashes so short that every probe is long and wraps.
oem_em_run_cells_records_whitelist_sparse is held to the five steps it replaces -- oem_correct_barcodes, the rejected
records dropped on the host, the labels' bytes as barcodes, oem_em_run_cells_records_umis_rule_sparse, the order mapped
back -- exactly in every index array and count, kept, the discard tables, cell_dups, cell_corrected and the columns, and
by tests/test_collate_gpu.py's _same_cells in the entries."""
import ctypes as C

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth, writers
from oarfish_amd.builder import ALN_RECORD, filters_c
from oarfish_amd.em import UmiRuleC, _discard_tables, _take_cells_result, gather_names
from tests.test_cells_records_gpu import COVS
from tests.test_cells_records_names_gpu import MODES, pack
from tests.test_collate_gpu import MAX_ITER, T
from tests.test_correct_barcodes import (ACGT, CORRECT, HOOK, NO_ID, ONE_CALL, RANDOM_SEEDS, _sub, all_cases, call_correct, host_walk,
                                         make_rule, random_case, restate_rule)
from tests.test_dedup_umis_gpu import _one_call as _umis_call, _same_umis
from tests.test_dedup_umis_rule_gpu import _one_call as _rule_call

pytestmark = pytest.mark.gpu

WHAT = ("id", "status", "order", "cell_rec_off", "counts")


# ---- oem_correct_barcodes ------------------------------------------------------------------------------------------------
def _check(case, multi, label, libs=None):
    want = host_walk(case, multi)
    for L in libs or (_lib.lib(), _lib.testing_lib()):
        rc, msg, *got = call_correct(L, CORRECT, case, multi, device=0)
        assert rc == _lib.OEM_OK, (label, msg)
        for k, what in enumerate(WHAT):
            assert got[k] == want[k], f"{label}: {what}"
    return want


def test_correct_equals_the_host_walk_on_the_cpu_cases():
    for label, case, multi in all_cases():
        _check(case, multi, label)
    rc, msg, *got = call_correct(_lib.lib(), CORRECT, all_cases()[0][1], 1, device=0, outs=False)     # every array output NULL
    assert rc == _lib.OEM_OK and (len(got[2]), len(got[3]) - 1) == (5, 1), msg


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_correct_equals_the_host_walk_on_the_random_cases(seed):
    case = random_case(seed)
    for multi in (0, 1):
        want = _check(case, multi, f"random {seed}, multi {multi}")
        assert want == restate_rule(case, multi)[0]


def _labels(n, length=12, seed=0):
    wl = synth.make_whitelist(n, length=length, seed=seed)
    return [wl[0][int(wl[1][w]):int(wl[1][w + 1])].tobytes() for w in range(n)]


def _one_off(label, rng, known):
    """`label` with one nucleotide substituted, not a label itself."""
    while True:
        p = int(rng.integers(0, len(label)))
        b = _sub(label, p, ACGT[(ACGT.index(label[p]) + int(rng.integers(1, 4))) % 4])
        if b not in known:
            return b


@pytest.mark.parametrize("n_labels", [1, 63, 64, 65, 4096, 4097])
def test_whitelist_sizes_around_the_launch_edges_and_the_tables_first_capacity(n_labels):
    """4096 labels fill the first table (8192 slots) to a half, 4097 take the next size."""
    rng = np.random.default_rng(n_labels)
    labels = _labels(n_labels, seed=n_labels)
    known = set(labels)
    bcs = []
    for k in range(300):
        lab = labels[(k * 7919) % n_labels] if k % 5 else labels[-1]          # the last label too: the insert's and lookup's last lane
        bcs.append(lab if k % 3 else _one_off(lab, rng, known))
    bcs += [labels[0], _one_off(labels[0], rng, known), b"", b"ACGT"]
    case = dict(whitelist=labels, barcodes=bcs)
    want = _check(case, 1, f"{n_labels} labels")
    assert want[4][0] >= 200 and want[4][1] >= 1
    if n_labels <= 65:   # (all pairs against thousands of labels take the walk here seconds; the host walk is held to it elsewhere)
        assert want == restate_rule(case, 1)[0]


@pytest.mark.parametrize("n_miss", [0, 1, 63, 64, 65, 255, 256, 257])
def test_miss_counts_around_the_wavefront_and_workgroup_edges(n_miss):
    """The misses are what the neighbour pass runs over, a wavefront each, four to a workgroup; their list is filled by
    one atomic per wavefront of the exact pass."""
    rng = np.random.default_rng(1000 + n_miss)
    labels = _labels(50, seed=77)
    known = set(labels)
    exact = [labels[int(rng.integers(0, 50))] for _ in range(130)]
    miss = [_one_off(labels[int(rng.integers(0, 50))], rng, known) if k % 4 else bytes(ACGT[x] for x in rng.integers(0, 4, size=12))
            for k in range(n_miss)]
    assert not known & set(miss)
    bcs = exact + miss
    bcs = [bcs[i] for i in rng.permutation(len(bcs))]
    at = [i for i, b in enumerate(bcs) if b not in known]
    if n_miss:                                                                # a miss in the first and in the last lane
        bcs[0], bcs[at[0]] = bcs[at[0]], bcs[0]
        last = len(bcs) - 1 if n_miss == 1 or at[-1] == 0 else at[-1]
        bcs[-1], bcs[last] = bcs[last], bcs[-1]
    bcs.insert(5, b"")
    case = dict(whitelist=labels, barcodes=bcs)
    want = _check(case, 1, f"{n_miss} misses")
    assert sum(want[4][1:4]) == n_miss and want[4][4] == 1


def test_nothing_and_one_record_accepted():
    labels = _labels(20, seed=5)
    none = dict(whitelist=labels, barcodes=[b"", b"NN", labels[0] + b"A", b"N" * 12, b""])
    want = _check(none, 1, "nothing accepted")
    assert want[2:4] == ([], [0]) and want[4] == [0, 0, 3, 0, 2]
    for k, one in enumerate((labels[7], _sub(labels[7], 11, ord("N")))):
        bcs = [b"", b"NN", b"N" * 12, b""]
        bcs.insert(k * 4, one)                                               # the one accepted record first, then last
        want = _check(dict(whitelist=labels, barcodes=bcs), 0, "one accepted")
        assert want[2:4] == ([k * 4], [0, 1]) and want[0][k * 4] == 7


@pytest.mark.parametrize("bits", ["0", "4"])
def test_short_hashes_make_every_probe_long_and_wrap(monkeypatch, bits):
    """OEM_BARCODE_HASH_BITS = 0: every label's home is the table's last slot; 4: the last sixteen."""
    monkeypatch.setenv("OEM_BARCODE_HASH_BITS", bits)
    monkeypatch.setenv("OEM_BARCODE_TABLE_SLOTS0", "2")
    case = random_case(RANDOM_SEEDS[0], n_labels=80, n_records=500)
    want = restate_rule(case, 1)[0]
    assert host_walk(case, 1) == want
    assert _check(case, 1, f"{bits} hash bits", libs=(_lib.testing_lib(),)) == want
    for label, hand, multi in all_cases():
        _check(hand, multi, f"{label}, {bits} hash bits", libs=(_lib.testing_lib(),))


def test_errors_found_on_the_device_name_the_right_label_pair_or_record():
    good = [b"ACGT", b"AAAA"]
    many = _labels(700, seed=9)
    twice = list(many)
    twice[650], twice[300], twice[20] = many[41], many[40], many[40]          # (20, 40), (20, 300), (41, 650): the smallest is (20, 40)
    zeros = [b"ACGT"] * 400
    zeros[333], zeros[130], zeros[399] = b"AC\x00T", b"\x00", b"ACG\x00"
    cases = ((dict(whitelist=[b"ACGT", b"AC\x00T", b"\x00CGT"], barcodes=good), "label 1 of the whitelist contains a 0 byte"),
             (dict(whitelist=many[:500] + [b"A\x00"] + many[500:] + [b"\x00"], barcodes=good), "label 500 of the whitelist contains a 0 byte"),
             (dict(whitelist=[b"ACGT", b"TTTT", b"GGGG", b"TTTT", b"ACGT", b"TTTT"], barcodes=good), "labels 0 and 4 of the whitelist are equal"),
             (dict(whitelist=twice, barcodes=good), "labels 20 and 40 of the whitelist are equal"),
             (dict(whitelist=[b"ACGT"], barcodes=[b"ACGT", b"", b"AC\x00T", b"\x00"]), "the barcode of record 2 contains a 0 byte"),
             (dict(whitelist=[b"ACGT"], barcodes=zeros), "the barcode of record 130 contains a 0 byte"),
             (dict(whitelist=[b"ACGT", b"ACGT", b"A\x00"], barcodes=[b"\x00"]), "label 2 of the whitelist contains a 0 byte"),
             (dict(whitelist=[b"ACGT", b"ACGT"], barcodes=[b"\x00"]), "labels 0 and 1 of the whitelist are equal"))
    for case, word in cases:
        for L, fn, device in ((_lib.lib(), CORRECT, 0), (_lib.testing_lib(), CORRECT, 0), (_lib.testing_lib(), HOOK, None)):
            rc, msg, *_ = call_correct(L, fn, case, 0, device=device)
            assert rc == _lib.OEM_ERR_ARG and fn in msg and word in msg, (word, msg)
    _check(dict(whitelist=good, barcodes=[b"ACGT", b"AAAT", b"ACGA"]), 0, "a good call after the errors")


def test_the_wrapper():
    wl = [b"AAAA", b"AATT", b"CCCC"]
    bcs = [b"", b"AATA", b"CCCC", b"AAAA", b"CCCA", b"AAAA", b"GGGG"]
    wl_id, status, order, cro, counts = oarfish_amd.correct_barcodes(bcs, wl, multi=True)
    assert (wl_id.dtype, status.dtype, order.dtype, cro.dtype, counts.dtype) == (np.uint32, np.uint8, np.uint32, np.uint64, np.uint64)
    assert wl_id.tolist() == [NO_ID, 0, 2, 0, 2, 0, NO_ID] and status.tolist() == [4, 1, 0, 0, 1, 0, 2]
    assert order.tolist() == [1, 3, 5, 2, 4] and cro.tolist() == [0, 3, 5] and counts.tolist() == [3, 2, 1, 0, 1]
    assert writers.cell_labels(wl, wl_id, order, cro) == ["AAAA", "CCCC"]
    assert oarfish_amd.correct_barcodes(bcs, wl)[1].tolist() == [4, 3, 0, 0, 1, 0, 2]
    assert oarfish_amd.correct_barcodes(bcs, pack(wl), alphabet="C")[0].tolist() == [NO_ID, NO_ID, 2, 0, 2, 0, NO_ID]


# ---- the one call and the join -------------------------------------------------------------------------------------------
def _raw(whitelist, multi, filters, txp_len, rec, names, sec, barcodes, umis, gene_of=None, correct=False, model=-1, mode="sort", outs=True,
         max_iter=MAX_ITER, lib=None):
    L = lib or _lib.lib()
    F = filters_c(filters)
    txp_len = np.ascontiguousarray(txp_len, dtype=np.uint64)
    rec = np.ascontiguousarray(rec, dtype=ALN_RECORD)
    one = np.zeros(1, dtype=np.uint8)
    (blob, off), (bc_blob, bc_off) = ((np.ascontiguousarray(p[0], dtype=np.uint8) if len(p[0]) else one, np.ascontiguousarray(p[1], dtype=np.uint64))
                                      for p in (names, barcodes))
    um_blob = um_off = None
    if umis is not None:
        um_blob, um_off = np.ascontiguousarray(umis[0], dtype=np.uint8) if len(umis[0]) else one, np.ascontiguousarray(umis[1], dtype=np.uint64)
    n = len(rec)
    if sec is not None:
        sec = np.ascontiguousarray(np.asarray(sec) != 0, dtype=np.uint8)
    gene = None if gene_of is None else np.ascontiguousarray(gene_of, dtype=np.uint32)
    umi_rule = UmiRuleC(None if gene is None else gene.ctypes.data, 0 if gene is None else len(gene), int(correct))
    rule, keep = make_rule(dict(whitelist=whitelist), multi)
    cov = COVS[model]
    o = dict(order=np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32), cell_rec_off=np.zeros(n + 1, dtype=np.uint64),
             group_off=np.zeros(n + 1, dtype=np.uint64), cell_group_off=np.zeros(n + 1, dtype=np.uint64),
             kept=np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32), cell_dups=np.full(max(n, 1), 2 ** 64 - 1, dtype=np.uint64),
             cell_corrected=np.full(max(n, 1), 2 ** 64 - 1, dtype=np.uint64), wl_id=np.full(max(n, 1), 0xEEEEEEEE, dtype=np.uint32),
             status=np.full(max(n, 1), 0xEE, dtype=np.uint8), counts=np.full(5, 2 ** 64 - 1, dtype=np.uint64))
    ng, ncell, nsurv = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    res = C.c_void_p(1)
    ptr = lambda k: o[k].ctypes.data if outs else None   # noqa: E731
    ref = lambda v: C.byref(v) if outs else None         # noqa: E731
    rc = getattr(L, ONE_CALL)(
        C.addressof(rule), C.addressof(umi_rule), C.addressof(F), txp_len.ctypes.data, len(txp_len), rec.ctypes.data if n else None, n,
        bc_blob.ctypes.data if n else None, bc_off.ctypes.data, blob.ctypes.data if n else None, off.ctypes.data,
        None if sec is None or not n else sec.ctypes.data, None if um_blob is None else um_blob.ctypes.data,
        None if um_off is None else um_off.ctypes.data, MODES[mode], cov["bin_width"] if cov else 0, model, cov["growth_rate"] if cov else 0.0, 0,
        max_iter, 1e-3, ptr("order"), ref(nsurv), ptr("cell_rec_off"), ref(ncell), ptr("group_off"), ref(ng), ptr("cell_group_off"), ptr("kept"),
        ptr("cell_dups"), ptr("cell_corrected"), ptr("wl_id"), ptr("status"), ptr("counts"), C.byref(res))
    del keep
    return rc, (L.oem_last_error() or b"").decode(), res, o, L, int(ng.value), int(ncell.value), int(nsurv.value), n


def _one_call(*a, dims=None, **kw):
    rc, msg, res, o, L, ng, nc, ns, n = _raw(*a, **kw)
    assert rc == _lib.OEM_OK and res.value, (rc, msg)
    if dims is not None:
        ng, nc, ns = dims
    tables = _discard_tables(L, res, nc)
    cells = _take_cells_result(res, nc, L)
    return dict(order=o["order"][:ns], n_survivors=ns, cell_rec_off=o["cell_rec_off"][:nc + 1], group_off=o["group_off"][:ng + 1], n_groups=ng,
                cell_group_off=o["cell_group_off"][:nc + 1], kept=o["kept"][:ng], tables=tables, cells=cells, n_cells=nc,
                cell_dups=o["cell_dups"][:nc], cell_corrected=o["cell_corrected"][:nc], wl_id=o["wl_id"][:n], status=o["status"][:n],
                counts=o["counts"])


def _join(whitelist, multi, filters, txp_len, rec, names, sec, barcodes, umis, gene_of=None, correct=False, model=-1, mode="sort",
          max_iter=MAX_ITER):
    """The five steps, composed from the existing calls."""
    rec = np.ascontiguousarray(rec, dtype=ALN_RECORD)
    wl_id, status, _, _, counts = oarfish_amd.correct_barcodes(barcodes, whitelist, multi=bool(multi))
    keep = np.flatnonzero(wl_id != NO_ID)
    um = (np.zeros(0, dtype=np.uint8), np.zeros(len(keep) + 1, dtype=np.uint64)) if umis is None else gather_names(umis, keep)
    if len(keep):
        got = _rule_call(filters, txp_len, rec[keep], gather_names(names, keep), None if sec is None else np.asarray(sec)[keep],
                         gather_names(pack(whitelist), wl_id[keep]), um, gene_of, correct, model=model, mode=mode, max_iter=max_iter)
    else:   # (that helper hands the call its arrays' addresses whatever their size: no records, no call)
        got = None
    if got is not None:
        got["order"] = keep.astype(np.uint32)[got["order"]]
        got.update(wl_id=wl_id, status=status, counts=counts, keep=keep)
    return got


def _same_whitelist(got, want, label, outs=True):
    _same_umis(got, want, label, outs)
    if outs:
        for k in ("cell_corrected", "wl_id", "status", "counts"):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), f"{label}: {k}"


N_CELLS, N_BAD_CELLS, READS_PER_CELL = 4, 2, 200


@pytest.fixture(scope="module")
def raw_input():
    """Four cells of about 200 reads and two small ones whose barcodes are on no whitelist, interleaved; UMIs with PCR
    duplicates and errors; sequencing errors in the barcodes, the same on all records of a read.  Records 0 and n - 1 are
    rejected and carry what would be an error on an accepted record: a ref_id beyond the annotation and a 0 byte in the
    UMI on record 0, an empty name on record n - 1."""
    reads = [READS_PER_CELL + 7 * k for k in range(N_CELLS)] + [40, 25]
    stores = [synth.make_cells(1, r, T, kbar=4.0, seed=901 + k) for k, r in enumerate(reads)]
    co, rps, tids, ps, nnz = [0], [np.zeros(1, dtype=np.uint64)], [], [], 0
    for _, rp, tid, p in stores:
        rps.append(rp[1:] + np.uint64(nnz))
        tids.append(tid)
        ps.append(p)
        nnz += len(tid)
        co.append(co[-1] + len(rp) - 1)
    cr = synth.make_cell_records((np.array(co, dtype=np.uint64), np.concatenate(rps), np.concatenate(tids), np.concatenate(ps)), T, seed=13)
    rec, names, sec, cro = synth.shuffle_cell_records(cr, seed=3, style="illumina")
    whitelist = _labels(96, length=16, seed=21)
    cell_bc = whitelist[10:10 + N_CELLS] + [b"GGGGGGNNGGGGGGGG", whitelist[3][:15]]       # two Ns; a length no label has
    r1, n1, s1, bc1, _ = synth.interleave_cells(rec, names, sec, cro, cell_bc, seed=5, how="uniform")
    r2, n2, s2, bc2, umis, copies = synth.add_umi_duplicates(r1, n1, s1, bc1, rate=0.3, seed=17)
    umis = synth.add_umi_errors(umis, 0.2, seed=8, names=n2, barcodes=bc2)
    clean = bc2
    bc3 = synth.add_barcode_errors(bc2, 0.15, 0.05, seed=7, names=n2)
    n = len(r2)
    as_list = lambda p: [np.asarray(p[0]).tobytes()[int(p[1][i]):int(p[1][i + 1])] for i in range(n)]   # noqa: E731
    bcs, nms, ums = as_list(bc3), as_list(n2), as_list(umis)
    bcs[0], bcs[n - 1] = b"NNNNNNNNNNNNNNNN", b""
    nms[n - 1] = b""
    ums[0] = b"AC\x00T"
    r2 = r2.copy()
    r2["ref_id"][0] = T + 5
    gene_of = synth.gene_of_txps(T)
    return dict(filters=cr.filters, txp_len=cr.txp_len, rec=r2, names=pack(nms), sec=s2, barcodes=pack(bcs), umis=pack(ums), clean=clean,
                clean_names=n2, clean_umis=umis, whitelist=whitelist, gene_of=gene_of, n=n, joins={})


def _args(fx, umis=True):
    return fx["filters"], fx["txp_len"], fx["rec"], fx["names"], fx["sec"], fx["barcodes"], fx["umis"] if umis else None


VARIANTS = {"no umis": dict(umis=False), "umis": dict(umis=True), "umis under a rule": dict(umis=True, rule=True)}


def _ref(fx, variant, model, mode, multi=1):
    key = (variant, model, mode, multi)
    if key not in fx["joins"]:
        v = VARIANTS[variant]
        kw = dict(gene_of=fx["gene_of"], correct=True) if v.get("rule") else {}
        ref = _join(fx["whitelist"], multi, *_args(fx, v["umis"]), model=model, mode=mode, **kw)
        n, st = fx["n"], ref["status"]
        # the input exercises what the call adds: rejected records first and last, whole cells rejected, every status
        assert ref["wl_id"][0] == NO_ID and ref["wl_id"][n - 1] == NO_ID and ref["n_cells"] == N_CELLS
        assert all(int((st == k).sum()) >= 5 for k in (0, 1, 2)) and int((st == 4).sum()) >= 1 and ref["counts"][1] >= 30
        assert 0 < len(ref["keep"]) < n - 60 and int((ref["kept"] > 0).sum()) > 0.5 * len(ref["kept"]), "the filter dropped the reads"
        if v["umis"]:
            assert int(ref["cell_dups"].sum()) > 50, "nothing is deduplicated"
        if v.get("rule"):
            assert int(ref["cell_corrected"].sum()) > 5, "no UMI is corrected"
        fx["joins"][key] = ref
    return fx["joins"][key]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("model", [-1, 1])
@pytest.mark.parametrize("mode", ["sort", "adjacent"])
def test_the_one_call_equals_the_join(raw_input, mode, model, variant):
    fx, v = raw_input, VARIANTS[variant]
    kw = dict(gene_of=fx["gene_of"], correct=True) if v.get("rule") else {}
    got = _one_call(fx["whitelist"], 1, *_args(fx, v["umis"]), model=model, mode=mode, **kw)
    _same_whitelist(got, _ref(fx, variant, model, mode), f"{variant}, {mode}, model {model}")


def test_the_one_call_under_multi_0_and_without_outputs(raw_input):
    fx = raw_input
    want = _ref(fx, "umis", -1, "sort", multi=0)
    _same_whitelist(_one_call(fx["whitelist"], 0, *_args(fx), lib=_lib.testing_lib()), want, "multi 0, the testing library")
    dims = (want["n_groups"], want["n_cells"], want["n_survivors"])
    _same_whitelist(_one_call(fx["whitelist"], 0, *_args(fx), outs=False, dims=dims), want, "multi 0, no outputs", outs=False)


def test_what_would_be_an_error_on_an_accepted_record(raw_input):
    """The rejected records 0 and n - 1 carry a bad ref_id, a 0 byte in the UMI and an empty name (the fixture); on an
    accepted record each of them is the umis call's error, naming the record by its input index."""
    fx = raw_input
    want = _ref(fx, "umis", -1, "sort")
    k = int(want["keep"][len(want["keep"]) // 2])                            # an accepted record in the middle of the input
    n = fx["n"]
    as_list = lambda p: [np.asarray(p[0]).tobytes()[int(p[1][i]):int(p[1][i + 1])] for i in range(n)]   # noqa: E731
    names, umis = as_list(fx["names"]), as_list(fx["umis"])
    a = list(_args(fx))
    for what, at, value, word in (("name", 3, names[:k] + [b""] + names[k + 1:], f"record {k} has an empty name"),
                                  ("name", 3, names[:k] + [b"a\x00b"] + names[k + 1:], f"the name of record {k} contains a 0 byte"),
                                  ("umi", 6, umis[:k] + [b"A\x00"] + umis[k + 1:], f"the UMI of record {k} contains a 0 byte")):
        b = list(a)
        b[at] = pack(value)
        rc, msg, res, *_ = _raw(fx["whitelist"], 1, *b)
        assert rc == _lib.OEM_ERR_ARG and not res.value and ONE_CALL in msg and word in msg, (what, msg)
    head = int(want["order"][want["group_off"][5]])                           # the first record of a read that is kept
    rec = fx["rec"].copy()
    rec["ref_id"][head] = T + 1
    rec["flags"][head] &= ~np.uint32(_lib.REC_UNMAPPED)
    b = list(a)
    b[2] = rec
    rc, msg, res, *_ = _raw(fx["whitelist"], 1, *b)
    assert rc == _lib.OEM_ERR_ARG and not res.value and f"record {head}: ref_id {T + 1} is not below n_txps" in msg, msg
    _same_whitelist(_one_call(fx["whitelist"], 1, *a), want, "a good call after the errors")


def test_input_that_is_rejected_entirely_gives_no_cells(raw_input):
    fx = raw_input
    n = fx["n"]
    junk = pack([b"N" * 16 if i % 3 else b"" for i in range(n)])
    a = list(_args(fx))
    a[5] = junk
    assert _join(fx["whitelist"], 1, *a) is None                              # nothing is accepted: the join has nothing to call
    for umis in (True, False):
        a[6] = fx["umis"] if umis else None
        got = _one_call(fx["whitelist"], 1, *a)
        assert got["n_cells"] == 0 and got["n_groups"] == 0 and got["n_survivors"] == 0 and got["tables"] == []
        assert got["cell_rec_off"].tolist() == [0] and got["group_off"].tolist() == [0] and got["cell_group_off"].tolist() == [0]
        assert got["cells"][0].tolist() == [0] and len(got["cells"][1]) == 0 and len(got["cells"][2]) == 0
        assert (got["wl_id"] == NO_ID).all() and got["counts"].tolist() == [0, 0, n - (n + 2) // 3, 0, (n + 2) // 3]
    _one_call(fx["whitelist"], 1, *a, outs=False, dims=(0, 0, 0))


def test_whitelisted_input_gives_the_rule_calls_result_exactly(raw_input):
    fx = raw_input
    n = fx["n"]
    labels = fx["whitelist"]
    clean = [np.asarray(fx["clean"][0]).tobytes()[int(fx["clean"][1][i]):int(fx["clean"][1][i + 1])] for i in range(n)]
    bcs = pack([b if b in set(labels) else labels[50 + len(b) % 2] for b in clean])      # the two other cells get labels too
    a = (fx["filters"], fx["txp_len"], fx["rec"][1:], gather_names(fx["clean_names"], np.arange(1, n)), fx["sec"][1:],
         gather_names(bcs, np.arange(1, n)), gather_names(fx["clean_umis"], np.arange(1, n)))      # (record 0 has the bad ref_id)
    want = _rule_call(*a, fx["gene_of"], True)
    got = _one_call(labels, 1, *a, gene_of=fx["gene_of"], correct=True)
    _same_umis(got, want, "whitelisted input")
    assert np.array_equal(got["cell_corrected"], want["cell_corrected"]) and got["n_cells"] == N_CELLS + N_BAD_CELLS
    assert (got["status"] == 0).all() and got["counts"].tolist() == [n - 1, 0, 0, 0, 0]
    wl_id, status, order, cro, counts = oarfish_amd.correct_barcodes(a[5], labels)
    order_bc, cro_bc = oarfish_amd.collate_barcodes(a[5])
    assert np.array_equal(order, order_bc) and np.array_equal(cro, cro_bc) and order.dtype == order_bc.dtype and cro.dtype == cro_bc.dtype
    assert writers.cell_labels(labels, wl_id, order, cro) == writers.cell_barcodes(a[5], order_bc, cro_bc)


def test_the_wrapper_with_and_without_a_whitelist(raw_input):
    fx = raw_input
    f, tl, rec, names, sec, barcodes, umis = _args(fx)
    common = dict(names=names, secondary=sec, barcodes=barcodes, max_iter=MAX_ITER)
    kw = dict(umis=umis, gene_of=fx["gene_of"], umi_correct=True, whitelist=fx["whitelist"], barcode_multi=True)
    dev = oarfish_amd.em_cells_records_sparse(f, tl, rec, None, None, collate="device", **common, **kw)
    host = oarfish_amd.em_cells_records_sparse(f, tl, rec, None, None, collate="host", **common, **kw)
    want = _ref(fx, "umis under a rule", -1, "sort")
    assert len(dev) == len(host) == 13
    for got in (dev, host):
        d = dict(cells=got[:4], kept=got[4], tables=got[5], order=got[6], cell_rec_off=got[7], cell_dups=got[8], cell_corrected=got[9],
                 wl_id=got[10], status=got[11], counts=got[12], n_cells=len(got[7]) - 1, n_survivors=len(got[6]), n_groups=len(got[4]),
                 group_off=want["group_off"], cell_group_off=want["cell_group_off"])
        _same_whitelist(d, want, "the wrapper")
    no_umis = oarfish_amd.em_cells_records_sparse(f, tl, rec, None, None, collate="device", whitelist=fx["whitelist"], barcode_multi=True, **common)
    assert len(no_umis) == 13 and np.array_equal(no_umis[6], _ref(fx, "no umis", -1, "sort")["order"]) and not no_umis[8].any()
    # whitelist=None changes nothing: the UMIs form on corrected barcodes, as it was
    clean = (f, tl, rec[1:fx["n"] - 1], gather_names(fx["clean_names"], np.arange(1, fx["n"] - 1)), sec[1:fx["n"] - 1],
             gather_names(fx["clean"], np.arange(1, fx["n"] - 1)), gather_names(fx["clean_umis"], np.arange(1, fx["n"] - 1)))
    plain = oarfish_amd.em_cells_records_sparse(clean[0], clean[1], clean[2], None, None, collate="device", names=clean[3], secondary=clean[4],
                                                barcodes=clean[5], umis=clean[6], max_iter=MAX_ITER, whitelist=None)
    ref = _umis_call(*clean)
    assert len(plain) == 9
    d = dict(cells=plain[:4], kept=plain[4], tables=plain[5], order=plain[6], cell_rec_off=plain[7], cell_dups=plain[8],
             n_cells=len(plain[7]) - 1, n_survivors=len(plain[6]), n_groups=len(plain[4]), group_off=ref["group_off"],
             cell_group_off=ref["cell_group_off"])
    _same_umis(d, ref, "whitelist=None")
