"""GPU tests of the barcode collation.  oem_collate_barcodes is held to the host walk of oem_collate.h's barcode rule
(the testing library's oem_test_collate_barcodes_host) and to the NumPy oracle of tests/test_collate_barcodes.py;
oem_em_run_cells_records_barcodes_sparse to the four steps it replaces -- oem_collate_barcodes, the host gathers,
oem_em_run_cells_records_names_sparse, the composed order -- exactly in order, cell_rec_off, group_off, n_groups,
cell_group_off, kept, the discard tables and the columns, and by tests/test_collate_gpu.py's _same_cells in the entries."""
import ctypes as C

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth, writers
from oarfish_amd.builder import ALN_RECORD, filters_c
from oarfish_amd.em import _discard_tables, _take_cells_result, gather_names
from tests.test_cells_paths_gpu import _last_paths
from tests.test_cells_records_gpu import COVS
from tests.test_cells_records_names_gpu import (EDGE_FILTERS, EDGE_T, MODES, _args, _edge_records, _one_call as _names_call, _same_exact,
                                                base, pack)   # noqa: F401  (base: the module's fixture)
from tests.test_collate_barcodes import bad_barcode_cases, barcode_cases, oracle
from tests.test_collate_gpu import MAX_ITER, T, _same_cells

pytestmark = pytest.mark.gpu

NAME = "oem_em_run_cells_records_barcodes_sparse"


# ---- oem_collate_barcodes ------------------------------------------------------------------------------------------------
def _collate(L, barcodes):
    blob, off = pack(barcodes)
    n = len(barcodes)
    order = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
    cro = np.full(n + 1, 2 ** 64 - 1, dtype=np.uint64)
    nc = C.c_uint64(0)
    if n and not len(blob):
        blob = np.zeros(1, dtype=np.uint8)
    rc = L.oem_collate_barcodes(blob.ctypes.data if n else None, off.ctypes.data, n, 0, order.ctypes.data, cro.ctypes.data, C.byref(nc))
    return rc, (L.oem_last_error() or b"").decode(), order[:n], cro[:int(nc.value) + 1]


def _host_walk(barcodes):
    L = _lib.testing_lib()
    blob, off = pack(barcodes)
    n = len(barcodes)
    order = np.zeros(max(n, 1), dtype=np.uint32)
    cro = np.zeros(n + 1, dtype=np.uint64)
    nc = C.c_uint64(0)
    rc = L.oem_test_collate_barcodes_host(blob.ctypes.data if n else None, off.ctypes.data, n, order.ctypes.data, cro.ctypes.data, C.byref(nc))
    assert rc == _lib.OEM_OK, L.oem_last_error()
    return order[:n], cro[:int(nc.value) + 1]


def _check_collate(barcodes, label):
    want_order, want_cro = _host_walk(barcodes)
    for L in (_lib.lib(), _lib.testing_lib()):
        rc, msg, order, cro = _collate(L, barcodes)
        assert rc == _lib.OEM_OK, (label, msg)
        assert np.array_equal(order, want_order) and np.array_equal(cro, want_cro), label
    return want_order, want_cro


def test_collate_barcodes_equals_the_host_walk_on_the_cpu_cases():
    for name, barcodes in barcode_cases().items():
        order, cro = _check_collate(barcodes, name)
        assert (order.tolist(), cro.tolist()) == oracle(barcodes), name


@pytest.mark.parametrize("n", [255, 256, 257, 65537])
def test_collate_barcodes_across_launch_and_scan_blocks(n):
    pool = synth.make_barcodes(max(n // 7, 1), "var" if n % 2 else "10x", seed=n)
    barcodes = [pool[i] for i in np.random.default_rng(n).integers(0, len(pool), size=n)]
    order, cro = _check_collate(barcodes, f"n = {n}")
    assert not np.array_equal(order, np.arange(n)) and len(cro) - 1 == len(set(barcodes))


def test_collate_barcodes_in_several_upload_chunks(monkeypatch):
    pool = synth.make_barcodes(300, "10x", seed=8)
    barcodes = [pool[i] for i in np.random.default_rng(8).integers(0, 300, size=4000)]
    want = _host_walk(barcodes)
    monkeypatch.setenv("OEM_COLLATE_CHUNK_BYTES", str(18 * 1000 + 5))      # 72 000 bytes: four chunks, cut inside the one cell
    with _lib.testing() as L:
        rc, msg, order, cro = _collate(L, barcodes)
        last = (C.c_double * 8)()
        assert L.oem_debug_collate_barcodes_last_call(last) == _lib.OEM_OK
    assert rc == _lib.OEM_OK, msg
    # at least three chunks; 18 bytes are at most three key rounds, fewer where the barcodes separate earlier (a run settles
    # as soon as its members are one barcode)
    assert last[1] >= 3 and 1 <= last[0] <= 3, list(last)
    assert np.array_equal(order, want[0]) and np.array_equal(cro, want[1])


def test_a_bad_barcode_is_named_by_its_first_record():
    for barcodes, at, zero in bad_barcode_cases():
        rc, msg, _, _ = _collate(_lib.lib(), barcodes)
        word = f"the barcode of record {at} contains a 0 byte" if zero else f"record {at} has an empty barcode"
        assert rc == _lib.OEM_ERR_ARG and word in msg and "oem_collate_barcodes" in msg, (at, zero, msg)
    _check_collate([b"AC", b"G", b"AC"], "a good call after the errors")


# ---- the one call and the join -------------------------------------------------------------------------------------------
def _raw(filters, txp_len, rec, names, sec, barcodes, model=-1, mode="sort", outs=True, max_iter=MAX_ITER, skip=()):
    L = _lib.lib()
    F = filters_c(filters)
    txp_len = np.ascontiguousarray(txp_len, dtype=np.uint64)
    rec = np.ascontiguousarray(rec, dtype=ALN_RECORD)
    blob, off = (np.ascontiguousarray(names[0], dtype=np.uint8), np.ascontiguousarray(names[1], dtype=np.uint64))
    bc_blob, bc_off = (np.ascontiguousarray(barcodes[0], dtype=np.uint8), np.ascontiguousarray(barcodes[1], dtype=np.uint64))
    n = len(rec)
    if sec is not None:
        sec = np.ascontiguousarray(np.asarray(sec) != 0, dtype=np.uint8)
    cov = COVS[model]
    o = dict(order=np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32), cell_rec_off=np.zeros(n + 1, dtype=np.uint64),
             group_off=np.zeros(n + 1, dtype=np.uint64), cell_group_off=np.zeros(n + 1, dtype=np.uint64),
             kept=np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32))
    ng, ncell = C.c_uint64(0), C.c_uint64(0)
    res = C.c_void_p(1)
    if n and not len(blob):
        blob = np.zeros(1, dtype=np.uint8)
    if n and not len(bc_blob):
        bc_blob = np.zeros(1, dtype=np.uint8)
    ptr = lambda k: o[k].ctypes.data if outs and k not in skip else None   # noqa: E731
    rc = getattr(L, NAME)(
        C.addressof(F), txp_len.ctypes.data, len(txp_len), rec.ctypes.data if n else None, n, bc_blob.ctypes.data if n else None,
        bc_off.ctypes.data, blob.ctypes.data if n else None, off.ctypes.data, None if sec is None or not n else sec.ctypes.data,
        MODES[mode], cov["bin_width"] if cov else 0, model, cov["growth_rate"] if cov else 0.0, 0, max_iter, 1e-3,
        ptr("order"), ptr("cell_rec_off"), C.byref(ncell) if outs and "n_cells" not in skip else None, ptr("group_off"),
        C.byref(ng) if outs and "n_groups" not in skip else None, ptr("cell_group_off"), ptr("kept"), C.byref(res))
    o["n_groups"], o["n_cells"] = int(ng.value), int(ncell.value)
    return rc, (L.oem_last_error() or b"").decode(), res, o, L, n


def _one_call(*a, n_cells=None, **kw):
    rc, msg, res, o, L, n = _raw(*a, **kw)
    assert rc == _lib.OEM_OK and res.value, (rc, msg)
    nc = o["n_cells"] if n_cells is None else n_cells
    tables = _discard_tables(L, res, nc)
    cells = _take_cells_result(res, nc, L)
    ng = o["n_groups"]
    return dict(order=o["order"][:n], cell_rec_off=o["cell_rec_off"][:nc + 1], group_off=o["group_off"][:ng + 1], n_groups=ng,
                cell_group_off=o["cell_group_off"][:nc + 1], kept=o["kept"][:ng], tables=tables, cells=cells, n_cells=nc)


def _join(filters, txp_len, rec, names, sec, barcodes, model=-1, mode="sort", max_iter=MAX_ITER):
    """The four steps: collate_barcodes, the host gathers, the names call, the composed order."""
    order_bc, cro = oarfish_amd.collate_barcodes(barcodes)
    rec = np.ascontiguousarray(rec, dtype=ALN_RECORD)
    got = _names_call(filters, txp_len, rec[order_bc], gather_names(names, order_bc), None if sec is None else np.asarray(sec)[order_bc], cro,
                      model=model, mode=mode, max_iter=max_iter)
    got["order_bc"] = order_bc
    got["order"] = order_bc[got["order"]]
    got["cell_rec_off"] = cro
    got["n_cells"] = len(cro) - 1
    return got


def _same(got, want, label, outs=True):
    if outs:
        assert got["n_cells"] == want["n_cells"] and got["cell_rec_off"].dtype == np.uint64, label
        assert np.array_equal(got["cell_rec_off"], want["cell_rec_off"]), f"{label}: cell_rec_off"
    _same_exact(got, want, label, outs)
    _same_cells(got["cells"], want["cells"], label)


@pytest.fixture(scope="module")
def inter(base):   # noqa: F811
    """The names fixture given barcodes and interleaved: (how, style, with_sec) -> the one call's arguments."""
    cache = {}

    def get(how, bstyle, with_sec=True, nstyle="illumina"):
        key = (how, bstyle, with_sec, nstyle)
        if key not in cache:
            f, tl, rec, names, sec, cro = _args(base, nstyle, with_sec)
            barcodes = synth.make_barcodes(len(cro) - 1, bstyle, seed=11)
            r2, n2, s2, bc, perm = synth.interleave_cells(rec, names, sec, cro, barcodes, seed=5, how=how)
            cache[key] = dict(args=(f, tl, r2, n2, s2, bc), cell_barcodes=barcodes, perm=perm, joins={})
        return cache[key]
    return get


def _ref(fx, model=-1):
    if model not in fx["joins"]:
        ref = _join(*fx["args"], model=model)
        n = len(ref["order"])
        assert not np.array_equal(ref["order_bc"], np.arange(n)), "order_bc is the identity: nothing is collated"
        assert int((ref["kept"] > 0).sum()) > (0.9 if fx["args"][4] is not None else 0.5) * len(ref["kept"]), "the filter dropped the reads"
        fx["joins"][model] = ref
    return fx["joins"][model]


@pytest.mark.parametrize("model", [-1, 1])
@pytest.mark.parametrize("with_sec", [True, False])
@pytest.mark.parametrize("bstyle", ["10x", "var"])
@pytest.mark.parametrize("how", ["uniform", "blocks"])
def test_the_one_call_equals_the_join(inter, how, bstyle, with_sec, model):
    fx = inter(how, bstyle, with_sec)
    _same(_one_call(*fx["args"], model=model), _ref(fx, model), f"{how}, {bstyle}, secondary {with_sec}, model {model}")


def test_collated_input_gives_todays_result(base):   # noqa: F811
    f, tl, rec, names, sec, cro = _args(base, "uuid")
    pool = synth.make_barcodes(len(cro) - 1, "10x", seed=2)
    cell_of = np.repeat(np.arange(len(cro) - 1), np.diff(cro.astype(np.int64)))
    barcodes = pack([pool[c] for c in cell_of])
    for model in (-1, 1):
        got = _one_call(f, tl, rec, names, sec, barcodes, model=model)
        want = _names_call(f, tl, rec, names, sec, cro, model=model)
        assert np.array_equal(got["cell_rec_off"], cro) and got["cell_rec_off"].dtype == cro.dtype
        _same_exact(got, want, f"collated input, model {model}")
        _same_cells(got["cells"], want["cells"], f"collated input, model {model}")


@pytest.mark.parametrize("workers", [1, 2])
def test_cuts_do_not_change_the_result(inter, workers, monkeypatch):
    fx = inter("uniform", "10x")
    want = _ref(fx)
    n_rec = np.diff(want["cell_rec_off"].astype(np.int64))
    monkeypatch.setenv("OEM_COLLATE_BATCH_RECORDS", str(int(n_rec.max()) + 1))
    monkeypatch.setenv("OEM_CELLS_GROUP_NNZ", str(int(n_rec.max()) - 1))
    monkeypatch.setenv("OEM_COLLATE_CHUNK_BYTES", "50000")
    monkeypatch.setenv("OEM_CELLS_WORKERS", str(workers))
    with _lib.testing():
        got = _one_call(*fx["args"])
        paths = _last_paths()
    assert len(paths) >= 3, paths
    _same(got, want, f"cuts, {workers} workers")


def _edge_check(names, sec, barcodes, label, mode="sort", seed=0):
    tl = np.full(EDGE_T, 2000, dtype=np.uint64)
    a = (EDGE_FILTERS, tl, _edge_records(len(names), seed), pack(names), sec, pack(barcodes))
    want = _join(*a, max_iter=20, mode=mode)
    _same(_one_call(*a, max_iter=20, mode=mode), want, label)
    return want


@pytest.mark.parametrize("n", [51, 52, 256, 257])
def test_record_counts_around_the_gather_workgroups(n):
    rng = np.random.default_rng(n)
    reads = [b"read/%d" % v for v in rng.integers(0, max(n // 3, 1), size=n)]
    sec = [int(x) for x in rng.integers(0, 2, size=n)]
    barcodes = [(b"AAC", b"AACGTTGCA", b"T")[v] for v in rng.integers(0, 3, size=n)]
    want = _edge_check(reads, sec, barcodes, f"{n} records", seed=n)
    assert want["n_cells"] == 3 and not np.array_equal(want["order_bc"], np.arange(n))


def test_gather_edges():
    rng = np.random.default_rng(4)
    # every byte alignment of the names gather: lengths 1 .. 17 in one input, twice over, in two interleaved cells and a cell of one
    names = [bytes(rng.integers(0x61, 0x7b, size=k).astype(np.uint8)) for k in list(range(1, 18)) * 2]
    barcodes = [b"solo" if i == 20 else (b"GG", b"GGA")[i % 2] for i in range(len(names))]
    want = _edge_check(names, None, barcodes, "name lengths 1 .. 17")
    assert want["n_cells"] == 3 and 1 in np.diff(want["cell_rec_off"].astype(np.int64))
    _edge_check(names, [i % 3 == 0 for i in range(len(names))], [b"one"] * len(names), "one cell holds everything")


def test_adjacent_on_cells_that_are_name_collated_inside():
    reads = {0: [b"a", b"a", b"b", b"c", b"c", b"c"], 1: [b"a", b"d", b"d"], 2: [b"zz"] * 4}
    deal = [0, 1, 0, 0, 2, 1, 2, 0, 0, 2, 1, 0, 2]      # the cells interleaved, each cell's names in collated order
    at = {c: 0 for c in reads}
    names, barcodes = [], []
    for c in deal:
        names.append(reads[c][at[c]])
        barcodes.append((b"ACGTACGTA", b"ACGTACGT", b"C")[c])
        at[c] += 1
    want = _edge_check(names, None, barcodes, "adjacent", mode="adjacent")
    assert np.array_equal(want["order"], want["order_bc"]) and want["n_groups"] == 3 + 2 + 1


# ---- errors found on the device, NULL outputs, the wrapper ---------------------------------------------------------------
def _fails(a, words, **kw):
    rc, msg, res, *_ = _raw(*a, **kw)
    assert rc == _lib.OEM_ERR_ARG and not res.value, (rc, msg)
    for w in words:
        assert w in msg, msg


def test_errors_found_on_the_device(inter):
    n = 700
    names = [b"read%05d" % (i * 7919 % 300) for i in range(n)]
    barcodes = [b"ACGTACGTAC%02d" % (i * 31 % 9) for i in range(n)]
    tl = np.full(EDGE_T, 2000, dtype=np.uint64)
    rec = _edge_records(n)
    good = (EDGE_FILTERS, tl, rec, pack(names), None, pack(barcodes))

    def check_good():
        _same(_one_call(*good, max_iter=20), _join(*good, max_iter=20), "a good call after an error")

    b2 = list(barcodes)
    b2[433], b2[650] = b"", b"AC\x00"
    _fails((EDGE_FILTERS, tl, rec, pack(names), None, pack(b2)), [NAME, "record 433 has an empty barcode"])
    check_good()
    b2[200] = b"ACGTACGT\x00C"
    _fails((EDGE_FILTERS, tl, rec, pack(names), None, pack(b2)), [NAME, "the barcode of record 200 contains a 0 byte"])
    check_good()
    n2 = list(names)
    n2[611], n2[305] = b"", b"re\x00d"
    for mode in ("sort", "adjacent"):
        _fails((EDGE_FILTERS, tl, rec, pack(n2), None, pack(barcodes)), [NAME, "the name of record 305 contains a 0 byte"], mode=mode)
    n2[12] = b""
    _fails((EDGE_FILTERS, tl, rec, pack(n2), None, pack(barcodes)), [NAME, "record 12 has an empty name"])
    check_good()
    # a bad ref_id, on the interleaved fixture: named by its index in the caller's input
    fx = inter("uniform", "10x")
    f, tl2, r2, n2, s2, bc = fx["args"]
    ref = _ref(fx)
    r2 = r2.copy()
    i = int(np.flatnonzero((r2["flags"] & _lib.REC_UNMAPPED) == 0)[1234])
    at = int(np.flatnonzero(ref["order"] == i)[0])
    c = int(np.searchsorted(ref["cell_rec_off"], at, side="right")) - 1
    r2["ref_id"][i] = T
    for filters in (f, dict(f, score_prob_denom=float("inf"))):     # ... and so does the host loop
        _fails((filters, tl2, r2, n2, s2, bc), [NAME, f"cell {c}:", f"record {i}:", f"ref_id {T} is not below n_txps"])
    _same_exact(_one_call(*fx["args"]), ref, "the fixture after the errors")


OUTPUTS = ["order", "cell_rec_off", "n_cells", "group_off", "n_groups", "cell_group_off", "kept"]


def test_null_outputs_give_the_same_result(inter):
    fx = inter("blocks", "var")
    want = _ref(fx)
    got = _one_call(*fx["args"], outs=False, n_cells=want["n_cells"])
    _same(got, want, "no outputs", outs=False)
    for k in OUTPUTS:
        got = _one_call(*fx["args"], skip=(k,), n_cells=want["n_cells"])
        for other in OUTPUTS:
            if other == k or other in ("group_off", "kept") and k == "n_groups" or other in ("cell_rec_off", "cell_group_off") and k == "n_cells":
                continue
            g = got[other][:len(want[other])] if isinstance(want[other], np.ndarray) else got[other]
            assert np.array_equal(g, want[other]), (k, other)
        _same(got, want, f"without {k}", outs=False)


def test_the_python_wrapper_returns_eight_values_on_both_paths(inter):
    fx = inter("uniform", "var")
    f, tl, rec, names, sec, bc = fx["args"]
    want = _ref(fx)
    run = lambda collate: oarfish_amd.em_cells_records_sparse(f, tl, rec, None, None, max_iter=MAX_ITER, conv_thresh=1e-3, names=names,   # noqa: E731
                                                              secondary=sec, barcodes=bc, collate=collate)
    dev, host = run("device"), run("host")
    assert len(dev) == 8 and len(host) == 8
    for g in (dev, host):
        assert np.array_equal(g[6], want["order"]) and np.array_equal(g[7], want["cell_rec_off"])
        assert np.array_equal(g[4], want["kept"]) and g[5] == want["tables"]
        _same_cells(g[:4], want["cells"], "wrapper")
    assert all(dev[k].dtype == host[k].dtype for k in (4, 6, 7))
    # the cells' barcodes, against the generator: cell c of the result is the cell whose record came first
    got = writers.cell_barcodes(bc, dev[6], dev[7])
    s = _args_cro = None   # noqa: F841
    first_seen = []
    blob, off = bc
    for k in range(len(rec)):
        b = bytes(blob[int(off[k]):int(off[k + 1])])
        if b not in first_seen:
            first_seen.append(b)
    assert got == [b.decode() for b in first_seen] and sorted(first_seen) == sorted(fx["cell_barcodes"])
