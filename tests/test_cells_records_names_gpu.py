"""GPU tests of the one call from names and records in input order (oem_em_run_cells_records_names_sparse): the collation,
the gather and the resident filter are held to the two calls the caller would otherwise join -- collate_names, then
em_cells_records_sparse on records[order] -- exactly in order, group_off, n_groups, cell_group_off, kept and the discard
tables, and by the rule tests/test_collate_gpu.py applies between these paths (_same_cells) in the entries and infos; the
filtered CSR is held to the host builder's export byte for byte."""
import ctypes as C

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth
from oarfish_amd.builder import ALN_RECORD, filters_c
from oarfish_amd.em import _discard_tables, _take_cells_result
from tests.test_cells_paths_gpu import _last_paths
from tests.test_cells_records_gpu import COVS, KEEP, READS, _host_way, _kept_csr, _split
from tests.test_collate import pack as _pack_names
from tests.test_collate_gpu import MAX_ITER, T, _same_cells

pytestmark = pytest.mark.gpu

NAME = "oem_em_run_cells_records_names_sparse"
MODES = {"sort": _lib.OEM_COLLATE_SORT, "adjacent": _lib.OEM_COLLATE_ADJACENT}
GATHER_WORKGROUP = 256     # k_records_gather: one lane per 8-byte word, five words per record


def pack(names):
    return _pack_names(names) if names else (np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))


# ---- the two sides ---------------------------------------------------------------------------------------------------
def _raw(filters, txp_len, rec, names, sec, cro, model=-1, mode="sort", outs=True, max_iter=MAX_ITER):
    """The C call as it is: (rc, message, result handle, outputs)."""
    L = _lib.lib()
    F = filters_c(filters)
    txp_len = np.ascontiguousarray(txp_len, dtype=np.uint64)
    rec = np.ascontiguousarray(rec, dtype=ALN_RECORD)
    blob, off = names
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    cro = np.ascontiguousarray(cro, dtype=np.uint64)
    n, n_cells = len(rec), len(cro) - 1
    if sec is not None:
        sec = np.ascontiguousarray(np.asarray(sec) != 0, dtype=np.uint8)
    cov = COVS[model]
    o = dict(order=np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32), group_off=np.zeros(n + 1, dtype=np.uint64),
             cell_group_off=np.zeros(n_cells + 1, dtype=np.uint64), kept=np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32))
    ng = C.c_uint64(0)
    res = C.c_void_p(1)
    if n and not len(blob):
        blob = np.zeros(1, dtype=np.uint8)
    rc = getattr(L, NAME)(
        C.addressof(F), txp_len.ctypes.data, len(txp_len), rec.ctypes.data if n else None, n, blob.ctypes.data if n else None,
        off.ctypes.data, None if sec is None or not n else sec.ctypes.data, cro.ctypes.data, n_cells, MODES[mode],
        cov["bin_width"] if cov else 0, model, cov["growth_rate"] if cov else 0.0, 0, max_iter, 1e-3,
        o["order"].ctypes.data if outs else None, o["group_off"].ctypes.data if outs else None, C.byref(ng) if outs else None,
        o["cell_group_off"].ctypes.data if outs else None, o["kept"].ctypes.data if outs else None, C.byref(res))
    o["n_groups"] = int(ng.value)
    return rc, (L.oem_last_error() or b"").decode(), res, o, L, n, n_cells


def _one_call(*a, **kw):
    rc, msg, res, o, L, n, n_cells = _raw(*a, **kw)
    assert rc == _lib.OEM_OK and res.value, (rc, msg)
    tables = _discard_tables(L, res, n_cells)
    cells = _take_cells_result(res, n_cells, L)
    ng = o["n_groups"]
    return dict(order=o["order"][:n], group_off=o["group_off"][:ng + 1], n_groups=ng, cell_group_off=o["cell_group_off"],
                kept=o["kept"][:ng], tables=tables, cells=cells)


def _two_step(filters, txp_len, rec, names, sec, cro, model=-1, mode="sort", max_iter=MAX_ITER):
    """What the caller joins today: collate_names, records[order] on the host, em_cells_records_sparse."""
    order, goff, cgo = oarfish_amd.collate_names(names, cro, sec, mode=mode)
    ref = oarfish_amd.em_cells_records_sparse(filters, txp_len, np.ascontiguousarray(rec, dtype=ALN_RECORD)[order], goff, cgo,
                                              coverage=COVS[model], max_iter=max_iter, conv_thresh=1e-3)
    return dict(order=order, group_off=goff, n_groups=len(goff) - 1, cell_group_off=cgo, kept=ref[4], tables=ref[5], cells=ref[:4])


def _same_exact(got, want, label, outs=True):
    if outs:
        assert got["n_groups"] == want["n_groups"], f"{label}: n_groups"
        for k in ("order", "group_off", "cell_group_off", "kept"):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), f"{label}: {k}"
    assert got["tables"] == want["tables"], f"{label}: discard tables"
    assert np.array_equal(got["cells"][0], want["cells"][0]) and np.array_equal(got["cells"][1], want["cells"][1]), f"{label}: columns"


def _same(got, want, label, outs=True):
    _same_exact(got, want, label, outs)
    _same_cells(got["cells"], want["cells"], label)


# ---- the end-to-end fixture of tests/test_collate_gpu.py, in both name styles ------------------------------------------
@pytest.fixture(scope="module")
def base():
    stores = [synth.make_cells(1, r, T, kbar=4.0, seed=201 + k, expressed_frac=0.1 if k % 2 else None) for k, r in enumerate(READS)]
    co, rps, tids, ps, nnz = [0], [np.zeros(1, dtype=np.uint64)], [], [], 0
    for _, rp, tid, p in stores:
        rps.append(rp[1:] + np.uint64(nnz))
        tids.append(tid)
        ps.append(p)
        nnz += len(tid)
        co.append(co[-1] + len(rp) - 1)
    cr = synth.make_cell_records((np.array(co, dtype=np.uint64), np.concatenate(rps), np.concatenate(tids), np.concatenate(ps)),
                                 T, seed=7)
    fx = dict(cr=cr, filters=cr.filters, txp_len=cr.txp_len, shuffled={}, refs={})
    for style in ("uuid", "illumina"):
        rec, names, sec, cro = synth.shuffle_cell_records(cr, seed=3, style=style)
        fx["shuffled"][style] = dict(rec=rec, names=names, sec=sec, cro=cro)
    return fx


def _args(base, style, with_sec=True):
    s = base["shuffled"][style]
    return base["filters"], base["txp_len"], s["rec"], s["names"], s["sec"] if with_sec else None, s["cro"]


def _ref(base, style, with_sec=True, model=-1):
    """The two-step path of the product library on the fixture, computed once and left alone."""
    key = (style, with_sec, model)
    if key not in base["refs"]:
        ref = _two_step(*_args(base, style, with_sec), model=model)
        n = len(ref["order"])
        assert not np.array_equal(ref["order"], np.arange(n)), "the order is the identity: nothing is gathered"
        # most reads are kept: nine in ten with the primaries marked, more than half where any record may lead its read
        assert int((ref["kept"] > 0).sum()) > (0.9 if with_sec else 0.5) * len(ref["kept"]), "the filter dropped the reads"
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        base["refs"][key] = ref
    return base["refs"][key]


# ---- 1. equals the two-step path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [-1, 1])
@pytest.mark.parametrize("with_sec", [True, False])
@pytest.mark.parametrize("style", ["uuid", "illumina"])
def test_equals_collate_then_records_call(base, style, with_sec, model):
    got = _one_call(*_args(base, style, with_sec), model=model)
    _same(got, _ref(base, style, with_sec, model), f"{style}, secondary {with_sec}, model {model}")


def test_the_python_wrapper_returns_the_host_paths_seven_values(base):
    f, tl, rec, names, sec, cro = _args(base, "illumina")
    want = _ref(base, "illumina")
    got = oarfish_amd.em_cells_records_sparse(f, tl, rec, None, cro, max_iter=MAX_ITER, conv_thresh=1e-3, names=names, secondary=sec,
                                              collate="device")
    host = oarfish_amd.em_cells_records_sparse(f, tl, rec, None, cro, max_iter=MAX_ITER, conv_thresh=1e-3, names=names, secondary=sec)
    assert len(got) == 7 and len(host) == 7
    for g in (got, host):
        assert np.array_equal(g[6], want["order"]) and np.array_equal(g[4], want["kept"]) and g[5] == want["tables"]
        _same_cells(g, want["cells"], "wrapper")
    assert got[4].dtype == host[4].dtype and got[6].dtype == host[6].dtype


# ---- 2. the filtered CSR is the builder's, byte for byte ---------------------------------------------------------------
@pytest.mark.parametrize("style", ["uuid", "illumina"])
def test_the_filtered_csr_is_the_builders_byte_for_byte(base, style, monkeypatch):
    want = _ref(base, style)
    f, tl, rec, names, sec, cro = _args(base, style)
    monkeypatch.setenv(KEEP, "1")
    with _lib.testing() as L:
        _one_call(f, tl, rec, names, sec, cro, max_iter=5)
        assert len(_last_paths()) == 1          # one group holds every cell
        rp, tid, p, s, e, cell_row_off = _kept_csr(L)
    host = _host_way(f, tl, _split(rec[want["order"]], want["group_off"], want["cell_group_off"]))
    want_rp, want_cro, nnz = [np.zeros(1, dtype=np.uint64)], [0], 0
    for h in host:
        want_rp.append(h["rp"][1:] + np.uint64(nnz))
        nnz += len(h["tid"])
        want_cro.append(want_cro[-1] + len(h["rp"]) - 1)
    assert nnz > 10000
    assert np.array_equal(rp.astype(np.uint64), np.concatenate(want_rp))
    assert np.array_equal(cell_row_off, np.array(want_cro, dtype=np.uint64))
    assert tid.tobytes() == np.concatenate([h["tid"] for h in host]).tobytes()
    assert p.tobytes() == np.concatenate([h["p"] for h in host]).tobytes()       # as_prob, bit for bit
    assert s.tobytes() == np.concatenate([h["s"] for h in host]).tobytes()
    assert e.tobytes() == np.concatenate([h["e"] for h in host]).tobytes()


# ---- 3. cuts do not change the result ----------------------------------------------------------------------------------
@pytest.mark.parametrize("workers,model", [(1, -1), (2, -1), (2, 1)])
def test_cuts_do_not_change_the_result(base, workers, model, monkeypatch):
    """Several groups of cells (one cell exceeds the bound and runs cell by cell), name chunks of a cell or two, one
    worker and two.  The two-step path under the same knobs makes the same cuts (the bound counts records on both)."""
    args = _args(base, "illumina")
    cro, off = args[5].astype(np.int64), args[3][1]
    n_rec = np.diff(cro)
    big = int(n_rec.argmax())
    per_cell_bytes = np.diff(off[cro].astype(np.int64))
    monkeypatch.setenv("OEM_CELLS_GROUP_NNZ", str(int(n_rec.max()) - 1))
    monkeypatch.setenv("OEM_COLLATE_CHUNK_BYTES", str(int(1.5 * np.median(per_cell_bytes))))
    monkeypatch.setenv("OEM_CELLS_WORKERS", str(workers))
    with _lib.testing():
        got = _one_call(*args, model=model)
        paths = _last_paths()
        same_knobs = _two_step(*args, model=model)
        assert _last_paths() == paths                # the same cuts on both sides
    assert len(paths) >= 3 and (big, big + 1, 0) in paths, paths
    assert sum(1 for _, _, b in paths if b) >= 2, paths
    assert paths[0][0] == 0 and paths[-1][1] == len(n_rec) and all(a[1] == b[0] for a, b in zip(paths, paths[1:]))
    label = f"cuts, {workers} workers, model {model}"
    _same(got, same_knobs, label)
    _same_exact(got, _ref(base, "illumina", True, model), label + " (against the uncut product call)")


def test_the_collation_bounds_cut_groups_too(base, monkeypatch):
    """A group of cells is one collation batch: the batch's record bound and the bound on a group's name bytes cut it,
    where the records call alone would have made one group.  What the filter and the collation give stays exact."""
    args = _args(base, "uuid")
    cro, off = args[5].astype(np.int64), args[3][1]
    want = _ref(base, "uuid")
    for knob, value in (("OEM_COLLATE_BATCH_RECORDS", int(np.diff(cro).max()) + 1),
                        ("OEM_CELLS_GROUP_NAME_BYTES", int(np.diff(off[cro].astype(np.int64)).max()) + 1)):
        with monkeypatch.context() as m:
            m.setenv(knob, str(value))
            with _lib.testing():
                got = _one_call(*args)
                paths = _last_paths()
        assert len(paths) >= 4, (knob, paths)
        _same(got, want, knob)


# ---- 4. edges ------------------------------------------------------------------------------------------------------------
EDGE_T = 40
EDGE_FILTERS = dict(five_prime_clip=2 ** 32 - 1, three_prime_clip=2 ** 62, score_threshold=0.95, min_aligned_fraction=0.5,
                    min_aligned_len=50, which_strand=0, score_prob_denom=5.0)


def _edge_records(n, seed=0):
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, dtype=ALN_RECORD)
    for i in range(n):
        rec[i] = (int(rng.integers(0, EDGE_T)), 10, 1500, 1400, 1000 - int(rng.integers(0, 30)), 1500, _lib.REC_HAS_SCORE, 0)
    return rec


def _edge_check(names, sec, cro, label, seed=0):
    tl = np.full(EDGE_T, 2000, dtype=np.uint64)
    rec = _edge_records(len(names), seed)
    a = (EDGE_FILTERS, tl, rec, pack(names), sec, np.array(cro, dtype=np.uint64))
    want = _two_step(*a, max_iter=20)
    _same(_one_call(*a, max_iter=20), want, label)
    _same(_one_call(*a, max_iter=20, outs=False), want, label + ", no outputs", outs=False)
    return want


def test_edges_in_one_hand_built_input():
    names = [b"solo",                                            # cell 2: one record
             b"same", b"same", b"same", b"same",                 # cell 3: one name, one group
             b"rr", b"aa", b"rr",                                # cell 5 ...
             b"rr", b"rr",                                       # ... and cell 6: the same name next door, two groups
             b"r10", b"r1/2", b"r1", b"r10", b"r1", b"r", b"r1/",  # cell 7: proper prefixes of one another
             b"late", b"late", b"early"]                         # cell 8: the secondary comes before its primary
    sec = [0, 0, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0, 0]
    cro = [0, 0, 0, 1, 5, 5, 8, 10, 17, 20, 20]                  # empty cells at the start, in the middle, at the end
    assert len(names) == len(sec) == cro[-1]
    want = _edge_check(names, sec, cro, "edges")
    assert list(want["cell_group_off"]) == [0, 0, 0, 1, 2, 2, 4, 5, 10, 12, 12]
    assert list(want["order"][17:20]) == [19, 18, 17]            # early, then late's primary before its secondary
    _edge_check(names, sec, [0, len(names)], "edges, n_cells = 1")
    _edge_check(names, None, cro, "edges, no secondary flags")


@pytest.mark.parametrize("n_cells", [1, 3])
def test_no_records(n_cells):
    want = _edge_check([], None, [0] * (n_cells + 1), f"no records, {n_cells} cells")
    assert want["n_groups"] == 0 and list(want["group_off"]) == [0] and len(want["cells"][1]) == 0


@pytest.mark.parametrize("n", [51, GATHER_WORKGROUP - 1, GATHER_WORKGROUP, GATHER_WORKGROUP + 1, 2 * GATHER_WORKGROUP, 2 * GATHER_WORKGROUP + 3])
def test_record_counts_around_the_gather_workgroup(n):
    """5 n words over workgroups of 256 lanes: a last workgroup that is full (n a multiple of 256) and one that is not."""
    rng = np.random.default_rng(n)
    reads = [b"read/%d" % v for v in rng.integers(0, max(n // 3, 1), size=n)]
    sec = [int(x) for x in rng.integers(0, 2, size=n)]
    assert (5 * n) % GATHER_WORKGROUP == 0 or n % GATHER_WORKGROUP
    want = _edge_check(reads, sec, [0, n // 2, n], f"{n} records", seed=n)
    assert not np.array_equal(want["order"], np.arange(n))


# ---- 5. adjacent -------------------------------------------------------------------------------------------------------
def test_adjacent_on_name_collated_input(base):
    f, tl, rec, names, sec, cro = _args(base, "illumina")
    ref = _ref(base, "illumina")
    order = ref["order"].astype(np.int64)
    blob, off = names
    sorted_names = pack([bytes(blob[int(off[i]):int(off[i + 1])]) for i in order])
    a = (f, tl, rec[order], sorted_names, sec[order], cro)
    got = _one_call(*a, mode="adjacent")
    assert np.array_equal(got["order"], np.arange(len(order), dtype=np.uint32))
    _same(got, _two_step(*a, mode="adjacent"), "adjacent")
    assert np.array_equal(got["group_off"], ref["group_off"]) and np.array_equal(got["kept"], ref["kept"])   # ... the sorted groups
    py = oarfish_amd.em_cells_records_sparse(f, tl, rec[order], None, cro, max_iter=MAX_ITER, conv_thresh=1e-3, names=sorted_names,
                                             collate="device", mode="adjacent")
    assert np.array_equal(py[6], got["order"]) and np.array_equal(py[4], got["kept"])


# ---- 6. the host loop ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["big_score", "inf_denom"])
def test_host_loop_fallbacks_on_shuffled_input(base, case):
    f, tl, rec, (blob, off), sec, cro = _args(base, "uuid")
    n = int(cro[6])                                              # the first six cells
    rec, sec, cro = rec[:n].copy(), sec[:n], cro[:7]
    names = (blob[:int(off[n])], off[:n + 1])
    filters = dict(f)
    if case == "big_score":
        i = int(cro[2]) + int(np.flatnonzero((rec["flags"][int(cro[2]):int(cro[3])] & _lib.REC_UNMAPPED) == 0)[5])
        rec["score"][i] = 2 ** 24 + 1
        rec["flags"][i] |= _lib.REC_HAS_SCORE
    else:
        filters["score_prob_denom"] = float("inf")
    a = (filters, tl, rec, names, sec, cro)
    want = _two_step(*a)
    assert not np.array_equal(want["order"], np.arange(n))
    _same(_one_call(*a), want, case)
    _same(_one_call(*a, outs=False), want, case + ", no outputs", outs=False)


# ---- 7. errors found on the device -------------------------------------------------------------------------------------
def _fails(a, code, words, **kw):
    rc, msg, res, *_ = _raw(*a, **kw)
    assert rc == code and not res.value, (rc, msg)
    for w in words:
        assert w in msg, msg


@pytest.mark.parametrize("mode", ["sort", "adjacent"])
def test_bad_names_are_found_on_the_device(mode):
    names = [b"read%05d" % (i * 7919 % 700) for i in range(700)]
    tl = np.full(EDGE_T, 2000, dtype=np.uint64)
    rec = _edge_records(700)
    cro = np.array([0, 300, 700], dtype=np.uint64)
    for bad, word in (([433, 650], "record 433 has an empty name"), ([131], "record 131 has an empty name")):
        n2 = list(names)
        for i in bad:
            n2[i] = b""
        _fails((EDGE_FILTERS, tl, rec, pack(n2), None, cro), _lib.OEM_ERR_ARG, [NAME, word], mode=mode)
    for bad, word in (([(433, 0), (650, 3)], "record 433 contains a 0 byte"), ([(699, 8)], "record 699 contains a 0 byte")):
        n2 = list(names)
        for i, at in bad:
            n2[i] = n2[i][:at] + b"\x00" + n2[i][at + 1:]
        rc, msg, res, *_ = _raw(EDGE_FILTERS, tl, rec, pack(n2), None, cro, mode=mode)
        assert rc == _lib.OEM_ERR_ARG and not res.value and word in msg.replace("the name of ", "") and NAME in msg, msg


@pytest.mark.parametrize("model", [-1, 1])
def test_a_bad_ref_id_is_named_by_its_input_index(base, model):
    f, tl, rec, names, sec, cro = _args(base, "illumina")
    ref = _ref(base, "illumina")
    rec = rec.copy()
    c = 2
    lo, hi = int(cro[c]), int(cro[c + 1])
    i = lo + int(np.flatnonzero((rec["flags"][lo:hi] & _lib.REC_UNMAPPED) == 0)[40])
    at = int(np.flatnonzero(ref["order"] == i)[0])
    assert at != i and lo <= at < hi                             # the collation moves it
    rec["ref_id"][i] = T
    _fails((f, tl, rec, names, sec, cro), _lib.OEM_ERR_ARG, [NAME, f"cell {c}:", f"record {i}:", f"ref_id {T} is not below n_txps"], model=model)
    filters = dict(f, score_prob_denom=float("inf"))             # ... and so does the host loop
    _fails((filters, tl, rec, names, sec, cro), _lib.OEM_ERR_ARG, [f"cell {c}:", f"record {i}:"], model=model)
    with pytest.raises(oarfish_amd.OemError) as ei:
        oarfish_amd.em_cells_records_sparse(f, tl, rec, None, cro, names=names, secondary=sec, collate="device")
    assert ei.value.code == _lib.OEM_ERR_ARG and f"record {i}:" in str(ei.value)


def test_an_alignment_outside_its_transcript_names_the_cell(base):
    f, tl, rec, names, sec, cro = _args(base, "illumina")
    ref = _ref(base, "illumina", True, 1)
    rec = rec.copy()
    c = 3
    g = int(ref["cell_group_off"][c]) + int(np.flatnonzero(ref["kept"][int(ref["cell_group_off"][c]):int(ref["cell_group_off"][c + 1])] == 1)[7])
    cand = [int(ref["order"][k]) for k in range(int(ref["group_off"][g]), int(ref["group_off"][g + 1]))]
    rec["aln_end"][cand] = 2 * tl[rec["ref_id"][cand]].astype(np.uint32)    # whichever record the read keeps: past the end
    assert _two_step(f, tl, rec, names, sec, cro, model=-1, max_iter=2)["kept"][g] == 1      # the filter still keeps it
    _fails((f, tl, rec, names, sec, cro), _lib.OEM_ERR_STATE, [f"cell {c}", "outside its transcript"], model=1)


# ---- 8. NULL outputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [-1, 1])
def test_null_outputs_give_the_same_result(base, model):
    got = _one_call(*_args(base, "uuid"), model=model, outs=False)
    assert got["n_groups"] == 0
    _same(got, _ref(base, "uuid", True, model), f"no outputs, model {model}", outs=False)
