"""GPU tests of the name collation (oem_collate_names, oem_collate_device.hip): every case checks order, group_off,
n_groups and cell_group_off for exact equality with the pure-Python oracle of tests/test_collate.py."""
import ctypes as C

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth
from oarfish_amd.builder import ALN_RECORD
from tests.common import f32_ulps
from tests.test_collate import ADJACENT, SORT, adjacent_cases, fixture_cases, oracle

pytestmark = pytest.mark.gpu

MODES = {SORT: "sort", ADJACENT: "adjacent"}


def _check(names, sec, cro, mode=SORT, label=""):
    """collate_names against the oracle; names: a list of bytes."""
    got = oarfish_amd.collate_names(names, cro, sec, mode=MODES[mode])
    order, goff, cgo = oracle(names, sec, cro, mode)
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint64 and got[2].dtype == np.uint64
    assert len(got[1]) - 1 == len(goff) - 1, f"{label}: n_groups"
    assert list(got[0]) == order, f"{label}: order"
    assert list(got[1]) == goff, f"{label}: group_off"
    assert list(got[2]) == cgo, f"{label}: cell_group_off"
    return got


def _last_call():
    out = (C.c_double * 8)()
    assert _lib.testing_lib().oem_debug_collate_last_call(out) == _lib.OEM_OK
    return dict(rounds=int(out[0]), chunks=int(out[1]), batches=int(out[2]), sorted_rounds=int(out[7]))


# ---- the cases of the CPU tier -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(fixture_cases()))
def test_key_edges_ties_and_cells(case):
    names, sec, cro = fixture_cases()[case]
    _check(names, sec, cro, SORT, case)
    _check(names, sec, cro, ADJACENT, case + ", adjacent")


def test_n_cells_1_and_both_libraries():
    names, sec, cro = fixture_cases()["one_read_scrambled"]
    assert len(cro) == 2
    _check(names, sec, cro)
    with _lib.testing():
        _check(names, sec, cro)


# ---- sizes across launch boundaries ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_sizes_across_launch_boundaries(n):
    rng = np.random.default_rng(n)
    distinct = [b"read/%d" % v for v in rng.permutation(n)]
    sec = [int(x) for x in rng.integers(0, 2, size=n)]
    _check(distinct, sec, [0, n], SORT, f"{n} distinct names")
    with _lib.testing():
        _check([b"the-one-read-name/1"] * n, sec, [0, n], SORT, f"{n} identical names")    # one group of n, and it ends
        assert _last_call()["rounds"] == 1                                                  # one name: settled at once


# ---- one larger case per name style, and the chunks ----------------------------------------------------------------------
def _larger(style):
    """64 cells of about 3 000 records; cell 10 is five cells' worth."""
    cells = synth.make_cells(68, 600, 400, kbar=4.0, seed=77)
    cr = synth.make_cell_records(cells, 400, seed=9)
    rec, (blob, off), sec, cro = synth.shuffle_cell_records(cr, seed=13, style=style)
    cro = np.delete(cro, [11, 12, 13, 14])
    names = [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(len(rec))]
    return dict(names=names, packed=(blob, off), sec=sec, cro=cro, want=oracle(names, sec, cro))


@pytest.fixture(scope="module", params=["uuid", "illumina"])
def larger(request):
    fx = _larger(request.param)
    n = np.diff(fx["cro"])
    assert len(n) == 64 and 2000 <= np.median(n) <= 4000, np.median(n)     # 64 cells x about 3 000 records
    assert fx["sec"].any() and not fx["sec"].all()
    fx["style"] = request.param
    return fx


def _check_larger(fx, label):
    got = oarfish_amd.collate_names(fx["packed"], fx["cro"], fx["sec"])
    order, goff, cgo = fx["want"]
    assert np.array_equal(got[0], np.array(order, dtype=np.uint32)), f"{label}: order"
    assert len(got[1]) == len(goff) and np.array_equal(got[1], np.array(goff, dtype=np.uint64)), f"{label}: group_off"
    assert np.array_equal(got[2], np.array(cgo, dtype=np.uint64)), f"{label}: cell_group_off"


def test_larger_case_and_its_rounds(larger):
    with _lib.testing():
        _check_larger(larger, larger["style"])
        info = _last_call()
    if larger["style"] == "illumina":
        assert info["rounds"] > 4, info      # 21 shared bytes, then lane, tile, x, y
    else:
        assert info["rounds"] <= 3, info
    assert info["chunks"] == 1 and info["batches"] == 1, info
    _check_larger(larger, larger["style"] + ", product library")


def test_chunks_do_not_change_the_result(larger, monkeypatch):
    """Upload chunks that hold 1 to 3 cells, with one cell larger than a chunk; then batches of a few cells as well."""
    per_cell = np.diff(larger["packed"][1][larger["cro"].astype(np.int64)]).astype(np.int64)
    chunk = int(3.2 * np.median(per_cell))
    assert per_cell.max() > chunk and np.sort(per_cell)[-2] * 2 < chunk
    monkeypatch.setenv("OEM_COLLATE_CHUNK_BYTES", str(chunk))
    with _lib.testing():
        _check_larger(larger, "chunks of 1 to 3 cells")
        info = _last_call()
    assert 22 <= info["chunks"] <= 40 and info["batches"] == 1, info
    monkeypatch.setenv("OEM_COLLATE_BATCH_RECORDS", str(int(np.median(np.diff(larger["cro"]))) * 5))
    with _lib.testing():
        _check_larger(larger, "chunks of 1 to 3 cells, batches of up to 5")
        info = _last_call()
    assert info["chunks"] >= 22 and 13 <= info["batches"] <= 32, info
    _check_larger(larger, "the product library has no knob")
    with _lib.testing():
        assert _last_call()["chunks"] >= 22      # (this thread's last call of the testing library: the one above)


# ---- adjacent ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(adjacent_cases()))
def test_adjacent(case):
    names, sec, cro = adjacent_cases()[case]
    got = _check(names, sec, cro, ADJACENT, case)
    assert list(got[0]) == list(range(len(names)))


def test_adjacent_on_the_sorted_input_gives_the_sorted_groups(larger):
    order, goff, cgo = larger["want"]
    names = [larger["names"][i] for i in order]
    got = oarfish_amd.collate_names(names, larger["cro"], None, mode="adjacent")
    assert np.array_equal(got[0], np.arange(len(names), dtype=np.uint32))
    assert list(got[1]) == goff and list(got[2]) == cgo


# ---- errors found on the device ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sort", "adjacent"])
def test_device_found_errors(mode):
    names = [b"read%05d" % i for i in range(700)]
    cro = [0, 300, 700]
    for bad, word in (([433, 650], b"record 433 has an empty name"), ([131], b"record 131 has an empty name")):
        n2 = list(names)
        for i in bad:
            n2[i] = b""
        with pytest.raises(_lib.OemError) as e:
            oarfish_amd.collate_names(n2, cro, mode=mode)
        assert e.value.code == _lib.OEM_ERR_ARG and word.decode() in str(e.value), str(e.value)
    for bad, word in (([(433, 0), (650, 3)], "record 433 contains a 0 byte"), ([(5, 8)], "record 5 contains a 0 byte"),
                      ([(699, 8)], "record 699 contains a 0 byte")):
        n2 = list(names)
        for i, at in bad:
            n2[i] = n2[i][:at] + b"\x00" + n2[i][at + 1:]
        with pytest.raises(_lib.OemError) as e:
            oarfish_amd.collate_names(n2, cro, mode=mode)
        assert e.value.code == _lib.OEM_ERR_ARG and word in str(e.value).replace("the name of ", ""), str(e.value)
    n2 = list(names)
    n2[40] = b""
    n2[20] = b"a\x00"
    with pytest.raises(_lib.OemError) as e:
        oarfish_amd.collate_names(n2, cro, mode=mode)
    assert "record 20 contains a 0 byte" in str(e.value).replace("the name of ", "")


# ---- end to end ----------------------------------------------------------------------------------------------------------
T = 600
MAX_ITER = 60


@pytest.fixture(scope="module")
def e2e():
    from tests.test_cells_records_gpu import READS
    stores = [synth.make_cells(1, r, T, kbar=4.0, seed=201 + k, expressed_frac=0.1 if k % 2 else None) for k, r in enumerate(READS)]
    co, rps, tids, ps, base = [0], [np.zeros(1, dtype=np.uint64)], [], [], 0
    for _, rp, tid, p in stores:
        rps.append(rp[1:] + np.uint64(base))
        tids.append(tid)
        ps.append(p)
        base += len(tid)
        co.append(co[-1] + len(rp) - 1)
    cr = synth.make_cell_records((np.array(co, dtype=np.uint64), np.concatenate(rps), np.concatenate(tids), np.concatenate(ps)),
                                 T, seed=7)
    rec, (blob, off), sec, cro = synth.shuffle_cell_records(cr, seed=3, style="illumina")
    names = [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(len(rec))]
    order, goff, cgo = oracle(names, sec, cro)
    order = np.array(order, dtype=np.int64)
    assert not np.array_equal(order, np.arange(len(rec)))
    ref = oarfish_amd.em_cells_records_sparse(cr.filters, cr.txp_len, rec[order], np.array(goff, dtype=np.uint64),
                                              np.array(cgo, dtype=np.uint64), max_iter=MAX_ITER, conv_thresh=1e-3)
    return dict(cr=cr, rec=rec, names=(blob, off), sec=sec, cro=cro, order=order, goff=goff, cgo=cgo, ref=ref)


def _same_cells(got, ref, label):
    indptr, cols, vals, infos = got[:4]
    assert np.array_equal(indptr, ref[0]) and np.array_equal(cols, ref[1]), f"{label}: columns"
    ulps = f32_ulps(vals, ref[2])
    assert ulps.max(initial=0) <= 1, f"{label}: {int(ulps.max())} f32 ulps"
    assert [(i.niter, bool(i.converged)) for i in infos] == [(i.niter, bool(i.converged)) for i in ref[3]], label


def test_records_call_with_names_equals_the_call_on_sorted_records(e2e):
    fx = e2e
    got = oarfish_amd.em_cells_records_sparse(fx["cr"].filters, fx["cr"].txp_len, fx["rec"], None, fx["cro"], max_iter=MAX_ITER,
                                              conv_thresh=1e-3, names=fx["names"], secondary=fx["sec"])
    assert len(got) == 7
    assert np.array_equal(got[6], fx["order"].astype(np.uint32))
    assert np.array_equal(got[4], fx["ref"][4])                       # kept, per group of the collated order
    assert got[5] == fx["ref"][5]                                     # every discard table
    _same_cells(got, fx["ref"], "records call")
    assert int((fx["ref"][4] > 0).sum()) > 0.9 * len(fx["ref"][4])   # (the filter kept most reads: the cells have entries)


def test_session_with_names_equals_the_call_on_sorted_records(e2e):
    fx = e2e
    cro = fx["cro"].astype(np.int64)
    blob, off = fx["names"]
    orders = []
    with oarfish_amd.CellsStream(T, max_iter=MAX_ITER, conv_thresh=1e-3, filters=fx["cr"].filters, txp_len=fx["cr"].txp_len) as s:
        for c in range(len(cro) - 1):
            a, b = cro[c], cro[c + 1]
            cell_names = (blob[int(off[a]):int(off[b])], off[a:b + 1] - off[a])
            ticket, order = s.push_records(fx["rec"][a:b], names=cell_names, secondary=fx["sec"][a:b])
            assert ticket == c
            orders.append(order.astype(np.int64) + a)
        got = s.finish()
        tables = s.discard_tables()
    assert np.array_equal(np.concatenate(orders), fx["order"])
    assert tables == fx["ref"][5]
    _same_cells(got, fx["ref"], "records session")


def test_defaults_are_unchanged(e2e):
    """Without names the records call takes grouped records as before and returns its six values."""
    fx = e2e
    got = oarfish_amd.em_cells_records_sparse(fx["cr"].filters, fx["cr"].txp_len, fx["rec"][fx["order"]],
                                              np.array(fx["goff"], dtype=np.uint64), np.array(fx["cgo"], dtype=np.uint64),
                                              max_iter=MAX_ITER, conv_thresh=1e-3)
    assert len(got) == 6 and np.array_equal(got[4], fx["ref"][4])
    with pytest.raises(ValueError):
        oarfish_amd.em_cells_records_sparse(fx["cr"].filters, fx["cr"].txp_len, fx["rec"], fx["goff"], fx["cgo"], secondary=fx["sec"])
