"""GPU tests of UMI deduplication.  oem_dedup_umis is held to the host walk of oem_collate.h's UMI rule (the testing
library's oem_test_dedup_umis_host) on the cases of tests/test_dedup_umis.py and at the launch, wavefront and scan-block
edges; oem_em_run_cells_records_umis_sparse to the seven steps it replaces -- oem_collate_barcodes, the host gathers,
oem_collate_names, the composed order, oem_dedup_umis, the duplicates dropped on the host, oem_em_run_cells_records_sparse
-- exactly in every index array and count, kept, the discard tables, cell_dups and the columns, and by
tests/test_collate_gpu.py's _same_cells in the entries; and to the existing barcodes call on the input before the
duplicates were added, cell by cell."""
import ctypes as C

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth, writers
from oarfish_amd.builder import ALN_RECORD, filters_c
from oarfish_amd.em import _discard_tables, _take_cells_result, gather_names
from tests.test_cells_paths_gpu import _last_paths
from tests.test_cells_records_gpu import COVS
from tests.test_cells_records_names_gpu import EDGE_FILTERS, EDGE_T, MODES, _edge_records, _same_exact, base, pack   # noqa: F401
from tests.test_collate_barcodes_gpu import _one_call as _barcodes_call, _same, inter   # noqa: F401  (base, inter: fixtures)
from tests.test_collate_gpu import MAX_ITER, T, _same_cells
from tests.test_dedup_umis import call_dedup, host_walk, make_case, umi_cases

pytestmark = pytest.mark.gpu

DEDUP = "oem_dedup_umis"
NAME = "oem_em_run_cells_records_umis_sparse"


# ---- oem_dedup_umis ------------------------------------------------------------------------------------------------------
def _check_dedup(case, label):
    want = host_walk(case)
    for L in (_lib.lib(), _lib.testing_lib()):
        rc, msg, *got = call_dedup(L, DEDUP, case, device=0)
        assert rc == _lib.OEM_OK, (label, msg)
        for k, what in enumerate(("dup", "survivor", "cell_dups")):
            assert got[k] == want[k], f"{label}: {what}"
    return want


def test_dedup_equals_the_host_walk_on_the_cpu_cases():
    for name, case in umi_cases().items():
        _check_dedup(case, name)


@pytest.mark.parametrize("ng", [1, 63, 64, 65, 255, 256, 257, 65537])
def test_group_counts_around_the_launch_wavefront_and_scan_edges(ng):
    umis = [b"UMI%09d" % (g * 7919 % ng) for g in range(ng)]        # 12 bytes, distinct: 7919 is prime and above no ng's factor
    assert len(set(umis)) == ng
    a, b = ng // 2, ng // 3
    if ng >= 4:
        umis[a], umis[ng - 1] = umis[0], umis[b]                     # two-member classes at the first and at the last group
    case = make_case([[[u] * (1 + g % 2) for g, u in enumerate(umis)]], seed=ng)
    dup, survivor, cell_dups = _check_dedup(case, f"{ng} groups")
    if ng >= 4:
        assert [g for g in range(ng) if dup[g]] == [a, ng - 1] and (survivor[a], survivor[ng - 1]) == (0, b) and cell_dups == [2]
    else:
        assert dup == [0] and cell_dups == [0]


def test_umis_longer_than_one_key():
    rng = np.random.default_rng(21)
    stem = b"ACGTACGTACGTACGT"                                        # 16 bytes: rounds 0 and 1 separate nothing
    pool = [stem + bytes(rng.integers(0x41, 0x45, size=int(rng.integers(1, 9))).astype(np.uint8)) for _ in range(40)]
    pool += [stem, stem[:8], stem[:9], pool[0][:17], pool[1] + b"A"]
    cells = [[[pool[int(rng.integers(0, len(pool)))]] * int(rng.integers(1, 4)) for _ in range(n)] for n in (150, 1, 149)]
    case = make_case(cells, seed=22)
    dup, _, cell_dups = _check_dedup(case, "long UMIs")
    assert sum(dup) > 200 and cell_dups[1] == 0


def test_dedup_in_several_batches_of_cells(monkeypatch):
    case = umi_cases()["three_cells_every_second_group_a_duplicate"]
    want = host_walk(case)
    monkeypatch.setenv("OEM_COLLATE_BATCH_RECORDS", "40")              # the cells hold 15, 192 and 99 records: three batches
    monkeypatch.setenv("OEM_COLLATE_CHUNK_BYTES", "64")
    with _lib.testing() as L:
        rc, msg, *got = call_dedup(L, DEDUP, case, device=0)
    assert rc == _lib.OEM_OK, msg
    assert tuple(got) == want and want[2] == [5, 64, 33] and max(want[1]) > 10 + 128


def test_dedup_errors_found_on_the_device():
    L = _lib.lib()
    case = make_case([[[b"ACGTAC"], [b"ACG\x00AC"], [b"ACGTAC"]], [[b"\x00"], [b"ACGTAC"]]], seed=None)
    rc, msg, *_ = call_dedup(L, DEDUP, case, device=0)
    assert rc == _lib.OEM_ERR_ARG and DEDUP in msg and "the UMI of record 1 contains a 0 byte" in msg, msg
    case = make_case([[[b"AC"], [b"AC"], [b"AC"]]], seed=None)
    case["order"] = [0, 7, 9]
    rc, msg, *_ = call_dedup(L, DEDUP, case, device=0)
    assert rc == _lib.OEM_ERR_ARG and DEDUP in msg and "order[1] = 7 is not below n_records = 3" in msg, msg
    _check_dedup(make_case([[[b"AC"], [b"G"], [b"AC"]]], seed=1), "a good call after the errors")
    dup, survivor, cell_dups = oarfish_amd.dedup_umis([b"AC", b"G", b"AC"], [0, 1, 2], [0, 1, 2, 3], [0, 3])
    assert (dup.tolist(), survivor.tolist(), cell_dups.tolist()) == ([0, 0, 1], [0, 1, 0], [1])
    assert (dup.dtype, survivor.dtype, cell_dups.dtype) == (np.uint8, np.uint64, np.uint64)


# ---- the one call and the join -------------------------------------------------------------------------------------------
def _raw(filters, txp_len, rec, names, sec, barcodes, umis, model=-1, mode="sort", outs=True, max_iter=MAX_ITER, skip=()):
    L = _lib.lib()
    F = filters_c(filters)
    txp_len = np.ascontiguousarray(txp_len, dtype=np.uint64)
    rec = np.ascontiguousarray(rec, dtype=ALN_RECORD)
    one = np.zeros(1, dtype=np.uint8)
    (blob, off), (bc_blob, bc_off), (um_blob, um_off) = (
        (np.ascontiguousarray(p[0], dtype=np.uint8) if len(p[0]) else one, np.ascontiguousarray(p[1], dtype=np.uint64))
        for p in (names, barcodes, umis))
    n = len(rec)
    if sec is not None:
        sec = np.ascontiguousarray(np.asarray(sec) != 0, dtype=np.uint8)
    cov = COVS[model]
    o = dict(order=np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32), cell_rec_off=np.zeros(n + 1, dtype=np.uint64),
             group_off=np.zeros(n + 1, dtype=np.uint64), cell_group_off=np.zeros(n + 1, dtype=np.uint64),
             kept=np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32), cell_dups=np.full(max(n, 1), 2 ** 64 - 1, dtype=np.uint64))
    ng, ncell, nsurv = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    res = C.c_void_p(1)
    ptr = lambda k: o[k].ctypes.data if outs and k not in skip else None   # noqa: E731
    ref = lambda k, v: C.byref(v) if outs and k not in skip else None      # noqa: E731
    rc = getattr(L, NAME)(
        C.addressof(F), txp_len.ctypes.data, len(txp_len), rec.ctypes.data if n else None, n, bc_blob.ctypes.data if n else None,
        bc_off.ctypes.data, blob.ctypes.data if n else None, off.ctypes.data, None if sec is None or not n else sec.ctypes.data,
        um_blob.ctypes.data, um_off.ctypes.data, MODES[mode], cov["bin_width"] if cov else 0, model, cov["growth_rate"] if cov else 0.0, 0,
        max_iter, 1e-3, ptr("order"), ref("n_survivors", nsurv), ptr("cell_rec_off"), ref("n_cells", ncell), ptr("group_off"),
        ref("n_groups", ng), ptr("cell_group_off"), ptr("kept"), ptr("cell_dups"), C.byref(res))
    o["n_groups"], o["n_cells"], o["n_survivors"] = int(ng.value), int(ncell.value), int(nsurv.value)
    return rc, (L.oem_last_error() or b"").decode(), res, o, L, n


def _one_call(*a, n_cells=None, n_survivors=None, **kw):
    rc, msg, res, o, L, n = _raw(*a, **kw)
    assert rc == _lib.OEM_OK and res.value, (rc, msg)
    nc = o["n_cells"] if n_cells is None else n_cells
    ns = o["n_survivors"] if n_survivors is None else n_survivors
    tables = _discard_tables(L, res, nc)
    cells = _take_cells_result(res, nc, L)
    ng = o["n_groups"]
    return dict(order=o["order"][:ns], n_survivors=ns, cell_rec_off=o["cell_rec_off"][:nc + 1], group_off=o["group_off"][:ng + 1], n_groups=ng,
                cell_group_off=o["cell_group_off"][:nc + 1], kept=o["kept"][:ng], tables=tables, cells=cells, n_cells=nc,
                cell_dups=o["cell_dups"][:nc])


def _join(filters, txp_len, rec, names, sec, barcodes, umis, model=-1, mode="sort", max_iter=MAX_ITER):
    """The seven steps: collate_barcodes, the host gathers, collate_names, the composed order, dedup_umis, the duplicates
    dropped on the host, the records call."""
    rec = np.ascontiguousarray(rec, dtype=ALN_RECORD)
    order_bc, cro = oarfish_amd.collate_barcodes(barcodes)
    order_names, goff, cgo = oarfish_amd.collate_names(gather_names(names, order_bc), cro, None if sec is None else np.asarray(sec)[order_bc],
                                                       mode=mode)
    order = order_bc[order_names]
    dup, survivor, cell_dups = oarfish_amd.dedup_umis(umis, order, goff, cgo, flags=rec["flags"])
    order2, goff2, cgo2, cro2 = oarfish_amd.drop_groups(order, goff, cgo, dup)
    ref = oarfish_amd.em_cells_records_sparse(filters, txp_len, rec[order2], goff2, cgo2, coverage=COVS[model], max_iter=max_iter,
                                              conv_thresh=1e-3)
    return dict(order=order2, n_survivors=len(order2), cell_rec_off=cro2, group_off=goff2, n_groups=len(goff2) - 1, cell_group_off=cgo2,
                kept=ref[4], tables=ref[5], cells=ref[:4], n_cells=len(cro2) - 1, cell_dups=cell_dups, dup=dup, survivor=survivor,
                full_order=order, full_group_off=goff)


def _same_umis(got, want, label, outs=True):
    if outs:
        assert got["n_survivors"] == want["n_survivors"], f"{label}: n_survivors"
        assert got["cell_dups"].dtype == want["cell_dups"].dtype and np.array_equal(got["cell_dups"], want["cell_dups"]), f"{label}: cell_dups"
    _same(got, want, label, outs)


@pytest.fixture(scope="module")
def aug(inter):   # noqa: F811
    """The interleaved fixture with UMIs and duplicates: with_sec -> the one call's arguments, the copy counts, the joins."""
    cache = {}

    def get(with_sec=True):
        if with_sec not in cache:
            fx = inter("uniform", "10x", with_sec)
            f, tl, rec, names, sec, bc = fx["args"]
            r2, n2, s2, b2, umis, copies = synth.add_umi_duplicates(rec, names, sec, bc, rate=0.3, seed=17)
            assert len(r2) > 1.2 * len(rec) and sum(copies.values()) > 2000
            cache[with_sec] = dict(args=(f, tl, r2, n2, s2, b2, umis), copies=copies, plain=fx, joins={})
        return cache[with_sec]
    return get


def _ref(fx, model=-1, mode="sort"):
    if (model, mode) not in fx["joins"]:
        ref = _join(*fx["args"], model=model, mode=mode)
        assert int(ref["dup"].sum()) > 2000 and ref["n_survivors"] < len(fx["args"][2]), "nothing is deduplicated"
        assert int((ref["kept"] > 0).sum()) > 0.5 * len(ref["kept"]), "the filter dropped the reads"
        fx["joins"][(model, mode)] = ref
    return fx["joins"][(model, mode)]


@pytest.mark.parametrize("model", [-1, 1])
@pytest.mark.parametrize("with_sec", [True, False])
@pytest.mark.parametrize("mode", ["sort", "adjacent"])
def test_the_one_call_equals_the_join(aug, mode, with_sec, model):
    fx = aug(with_sec)
    _same_umis(_one_call(*fx["args"], model=model, mode=mode), _ref(fx, model, mode), f"{mode}, secondary {with_sec}, model {model}")


def _by_barcode(barcodes, got):
    """barcode -> (columns, values, (niter, converged), sorted kept, cell_dups or None) of a result's cells."""
    labels = writers.cell_barcodes(barcodes, got["order"], got["cell_rec_off"])
    indptr, cols, vals, infos = got["cells"][:4]
    out = {}
    for c, b in enumerate(labels):
        g0, g1 = int(got["cell_group_off"][c]), int(got["cell_group_off"][c + 1])
        out[b] = (cols[indptr[c]:indptr[c + 1]], vals[indptr[c]:indptr[c + 1]], infos[c], np.sort(got["kept"][g0:g1]),
                  int(got["cell_dups"][c]) if "cell_dups" in got else None, got["tables"][c])
    assert len(out) == len(labels)
    return labels, out


def _as_cells(labels, per):
    """The cells of `per` in the order `labels`, as _same_cells takes them."""
    indptr = np.zeros(len(labels) + 1, dtype=np.int64)
    np.cumsum([len(per[b][0]) for b in labels], out=indptr[1:])
    return indptr, np.concatenate([per[b][0] for b in labels]), np.concatenate([per[b][1] for b in labels]), [per[b][2] for b in labels]


@pytest.mark.parametrize("with_sec", [True, False])
def test_the_cells_are_those_of_the_input_without_the_duplicates(aug, with_sec):
    fx = aug(with_sec)
    got = _one_call(*fx["args"])
    plain = _barcodes_call(*fx["plain"]["args"])                       # the existing call on the input before add_umi_duplicates
    labels, per = _by_barcode(fx["args"][5], got)
    plain_labels, plain_per = _by_barcode(fx["plain"]["args"][5], plain)
    assert sorted(labels) == sorted(plain_labels)
    assert [per[b][4] for b in labels] == [fx["copies"].get(b.encode("latin-1"), 0) for b in labels] and sum(got["cell_dups"]) > 2000
    for b in labels:
        assert np.array_equal(per[b][3], plain_per[b][3]) and per[b][5] == plain_per[b][5], b      # kept and the discard table
    _same_cells(_as_cells(labels, per), _as_cells(labels, plain_per), f"without the duplicates, secondary {with_sec}")


def test_empty_umis_give_the_barcodes_calls_result(aug):
    fx = aug()
    f, tl, rec, names, sec, bc, umis = fx["args"]
    want = _barcodes_call(f, tl, rec, names, sec, bc)
    no_umis = (np.zeros(0, dtype=np.uint8), np.zeros(len(rec) + 1, dtype=np.uint64))
    got = _one_call(f, tl, rec, names, sec, bc, no_umis)
    assert got["n_survivors"] == len(rec) and not got["cell_dups"].any() and len(got["cell_dups"]) == want["n_cells"]
    _same(got, want, "every UMI empty")
    # ... and umis=None is the barcodes entry: eight values
    run = lambda **kw: oarfish_amd.em_cells_records_sparse(f, tl, rec, None, None, max_iter=MAX_ITER, conv_thresh=1e-3, names=names,   # noqa: E731
                                                           secondary=sec, barcodes=bc, collate="device", **kw)
    none = run(umis=None)
    assert len(none) == 8 and np.array_equal(none[6], want["order"]) and np.array_equal(none[4], want["kept"])
    nine = run(umis=no_umis)
    assert len(nine) == 9 and np.array_equal(nine[6], want["order"]) and not nine[8].any()


def _strings(pair):
    raw, off = np.asarray(pair[0]).tobytes(), np.asarray(pair[1]).astype(np.int64)
    return [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def _surviving_reads(names, barcodes, got):
    """barcode -> the names of the reads a result kept in its collation, in collated order."""
    nm = _strings(names)
    heads = got["order"][got["group_off"][:-1].astype(np.int64)]
    labels = writers.cell_barcodes(barcodes, got["order"], got["cell_rec_off"])
    cgo = got["cell_group_off"].astype(np.int64)
    return {b: [nm[i] for i in heads[cgo[c]:cgo[c + 1]]] for c, b in enumerate(labels)}


@pytest.mark.parametrize("within_reads", ["kept", "shuffled"])
def test_a_permutation_of_the_input_gives_the_same_cells(aug, within_reads):
    """Under mode="sort" the survivor of a class is the read whose name sorts first, so which reads survive does not
    depend on the input's order: that is held under a uniform permutation of all records ("shuffled").  What the FILTER
    keeps of a read is a different matter.  It keeps the first of equal best scores (oem_filter.h: `score > best`), and the
    name rule orders a read's secondaries by input index, so a permutation that reorders a read's own secondaries may
    change that read's kept count with or without UMIs.  The columns and the kept multiset are therefore compared under a
    permutation that moves every record but keeps each read's records in their relative order ("kept")."""
    fx = aug()
    f, tl, rec, names, sec, bc, umis = fx["args"]
    ref = _ref(fx)
    want_labels, want = _by_barcode(bc, ref)
    n = len(rec)
    perm = np.random.default_rng(31).permutation(n)
    if within_reads == "kept":       # every read's records to the slots the permutation gave them, in their input order
        ids = {}
        rid = np.array([ids.setdefault(k, len(ids)) for k in zip(_strings(bc), _strings(names))], dtype=np.int64)
        pos = np.empty(n, dtype=np.int64)
        pos[perm] = np.arange(n)
        new_pos = np.empty(n, dtype=np.int64)
        new_pos[np.lexsort((np.arange(n), rid))] = pos[np.lexsort((pos, rid))]
        perm = np.argsort(new_pos)
        assert sorted(perm.tolist()) == list(range(n)) and (perm != np.arange(n)).mean() > 0.99
    a2 = (f, tl, rec[perm], gather_names(names, perm), np.asarray(sec)[perm], gather_names(bc, perm), gather_names(umis, perm))
    got_all = _one_call(*a2)
    labels, got = _by_barcode(a2[5], got_all)
    assert sorted(labels) == sorted(want_labels)
    assert _surviving_reads(a2[3], a2[5], got_all) == _surviving_reads(names, bc, ref)
    for b in labels:
        assert got[b][4] == want[b][4], f"{b}: cell_dups"
        if within_reads == "kept":
            assert np.array_equal(got[b][0], want[b][0]), f"{b}: columns"
            assert np.array_equal(got[b][3], want[b][3]) and got[b][5] == want[b][5], f"{b}: kept and the discard table"


@pytest.mark.parametrize("workers", [1, 2])
def test_cuts_do_not_change_the_result(aug, workers, monkeypatch):
    fx = aug()
    want = _ref(fx)
    # the records of the cells BEFORE the drop bound a group of cells: about one cell a group, so every class sits at a cut
    n_rec = np.diff(oarfish_amd.collate_barcodes(fx["args"][5])[1].astype(np.int64))
    monkeypatch.setenv("OEM_COLLATE_BATCH_RECORDS", str(int(n_rec.max()) + 1))
    monkeypatch.setenv("OEM_CELLS_GROUP_NNZ", str(int(n_rec.max()) - 1))
    monkeypatch.setenv("OEM_COLLATE_CHUNK_BYTES", "50000")
    monkeypatch.setenv("OEM_CELLS_WORKERS", str(workers))
    with _lib.testing():
        got = _one_call(*fx["args"])
        paths = _last_paths()
    assert len(paths) >= 3, paths
    _same_umis(got, want, f"cuts, {workers} workers")


def test_a_small_input_whose_classes_touch_every_boundary():
    # three cells dealt round-robin; in each, reads 0 and 1 (the first two groups) and the last two reads are one molecule
    n_reads, names, barcodes, umis = (5, 2, 7), [], [], []
    for r in range(max(n_reads)):
        for c, k in enumerate(n_reads):
            if r < k:
                for _ in range(1 + (r + c) % 2):
                    names.append(b"read%02d" % r)
                    barcodes.append((b"ACGTACGTA", b"ACGTACGT", b"C")[c])
                    umis.append(b"FIRST" if r < 2 else b"LAST" if r >= k - 2 else b"U%d" % r)
    tl = np.full(EDGE_T, 2000, dtype=np.uint64)
    for mode in ("sort", "adjacent"):
        a = (EDGE_FILTERS, tl, _edge_records(len(names), 3), pack(names), None, pack(barcodes), pack(umis))
        want = _join(*a, max_iter=20, mode=mode)
        assert want["cell_dups"].tolist() == [2, 1, 2] and want["n_groups"] == 3 + 1 + 5
        _same_umis(_one_call(*a, max_iter=20, mode=mode), want, f"small input, {mode}")


# ---- errors found on the device, NULL outputs, the wrapper ---------------------------------------------------------------
def _fails(a, words, **kw):
    rc, msg, res, *_ = _raw(*a, **kw)
    assert rc == _lib.OEM_ERR_ARG and not res.value, (rc, msg)
    for w in words:
        assert w in msg, msg


def test_errors_found_on_the_device(aug):
    fx = aug()
    f, tl, rec, names, sec, bc, umis = fx["args"]
    ref = _ref(fx)
    blob, off = np.array(umis[0]), umis[1].astype(np.int64)
    for i in (4321, 977):                                              # a 0 byte in two UMIs: the smaller index is named
        blob[off[i] + 5] = 0
    _fails((f, tl, rec, names, sec, bc, (blob, umis[1])), [NAME, "the UMI of record 977 contains a 0 byte"])
    # a bad ref_id in a surviving record: named by its cell and its index in the caller's input
    mapped = np.flatnonzero((rec["flags"] & _lib.REC_UNMAPPED) == 0)
    i = int(mapped[np.isin(mapped, ref["order"])][1234])
    at = int(np.flatnonzero(ref["order"] == i)[0])
    c = int(np.searchsorted(ref["cell_rec_off"], at, side="right")) - 1
    r2 = rec.copy()
    r2["ref_id"][i] = T
    for filters in (f, dict(f, score_prob_denom=float("inf"))):       # ... and so does the host loop
        _fails((filters, tl, r2, names, sec, bc, umis), [NAME, f"cell {c}:", f"record {i}:", f"ref_id {T} is not below n_txps"])
    # the same in a duplicate's record is never seen: its records are not gathered (and the join never gets them)
    g = int(np.flatnonzero(ref["dup"])[100])
    j = int(ref["full_order"][int(ref["full_group_off"][g])])
    assert j not in ref["order"]
    r3 = rec.copy()
    r3["ref_id"][j] = T
    _same_exact(_one_call(f, tl, r3, names, sec, bc, umis), ref, "a bad ref_id in a duplicate")
    _same_exact(_one_call(*fx["args"]), ref, "the fixture after the errors")


OUTPUTS = ["order", "n_survivors", "cell_rec_off", "n_cells", "group_off", "n_groups", "cell_group_off", "kept", "cell_dups"]
NEEDS = {"order": "n_survivors", "group_off": "n_groups", "kept": "n_groups", "cell_rec_off": "n_cells", "cell_group_off": "n_cells",
         "cell_dups": "n_cells"}


def test_null_outputs_give_the_same_result(aug):
    fx = aug(False)
    want = _ref(fx)
    sizes = dict(n_cells=want["n_cells"], n_survivors=want["n_survivors"])
    got = _one_call(*fx["args"], outs=False, **sizes)
    _same_umis(got, want, "no outputs", outs=False)
    for k in OUTPUTS:
        got = _one_call(*fx["args"], skip=(k,), **sizes)
        for other in OUTPUTS:
            if other == k or NEEDS.get(other) == k:
                continue
            g = got[other][:len(want[other])] if isinstance(want[other], np.ndarray) else got[other]
            assert np.array_equal(g, want[other]), (k, other)
        _same_umis(got, want, f"without {k}", outs=False)


def test_the_python_wrapper_returns_nine_values_on_both_paths(aug):
    fx = aug()
    f, tl, rec, names, sec, bc, umis = fx["args"]
    want = _ref(fx)
    run = lambda collate: oarfish_amd.em_cells_records_sparse(f, tl, rec, None, None, max_iter=MAX_ITER, conv_thresh=1e-3, names=names,   # noqa: E731
                                                              secondary=sec, barcodes=bc, umis=umis, collate=collate)
    dev, host = run("device"), run("host")
    assert len(dev) == 9 and len(host) == 9
    for g in (dev, host):
        assert np.array_equal(g[6], want["order"]) and np.array_equal(g[7], want["cell_rec_off"]) and np.array_equal(g[8], want["cell_dups"])
        assert np.array_equal(g[4], want["kept"]) and g[5] == want["tables"]
        _same_cells(g[:4], want["cells"], "wrapper")
    assert all(dev[k].dtype == host[k].dtype for k in (4, 6, 7, 8))
