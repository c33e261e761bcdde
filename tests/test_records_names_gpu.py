"""GPU tests of the bulk parser on the device (oem_store_create_records_names, DeviceStore.from_named_records,
bulk.quantify_bulk_alignments_from_records).

The reference of every test is the hand join the call replaces: drop the unmapped records, names and flags on the host,
``collate_names`` on what is left as one cell, ``records[order]``, ``DeviceStore.from_records`` -- and, for the parse
itself, the pure-Python oracle of tests/test_parse_names.py (the reference's ``prev_read`` state machine) and the host
walk of oem_collate.h (the testing library's oem_test_parse_bulk_host)."""
import ctypes as C

import numpy as np
import pytest

import oarfish_amd
from oarfish_amd import _lib, synth, writers
from oarfish_amd.em import gather_names
from oarfish_amd.builder import ALN_RECORD, StoreBuilder, filters_c
from oarfish_amd.types import DeviceStore, InMemoryAlignmentStore

from tests.common import assert_counts_close
from tests.test_collate import ADJACENT, SORT, pack
from tests.test_filter_groups_gpu import _compare
from tests.test_parse_names import FILTERS, NAME, NotCollated, T, UNMAPPED, bad_name_cases, oracle, parse_cases

pytestmark = pytest.mark.gpu
MODES = {ADJACENT: "adjacent", SORT: "sort"}
COVERAGE = {-1: None, 0: "logistic", 1: "binomial"}


# ---------------------------------------------------------------------------------------------------------------------
# the hand join
# ---------------------------------------------------------------------------------------------------------------------
def names_list(names):
    blob, off = names
    return [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def hand_join(F, txp_len, rec, names, sec, mode, coverage=None, **kw):
    """(store, order as input indices, group_off, kept, discard table) of the four steps the one call replaces."""
    idx = np.flatnonzero((rec["flags"] & UNMAPPED) == 0)
    order, group_off, _ = oarfish_amd.collate_names(gather_names(names, idx), [0, len(idx)], secondary=None if sec is None else sec[idx],
                                                    mode=MODES[mode])
    store, kept, dt = DeviceStore.from_records(F, txp_len, rec[idx][order], group_off, coverage=coverage, **kw)
    return store, idx[order], group_off, kept, dt


def check_outputs(parse, kept, dt, want, names, n_records, mode, check):
    """order, group_off, kept, the discard table, every info field and the row names against the hand join's."""
    _, w_order, w_group_off, w_kept, w_dt = want
    assert np.array_equal(parse.order, w_order) and np.array_equal(parse.group_off, w_group_off)
    assert np.array_equal(kept, w_kept) and dt == w_dt
    G = len(w_group_off) - 1
    assert (parse.n_unmapped, parse.n_parsed, parse.n_groups) == (n_records - len(w_order), len(w_order), G)
    assert (parse.n_reads, parse.unique_alignments) == (int(np.count_nonzero(w_kept)), int((w_kept == 1).sum()))
    assert parse.n_checked == (min(check, G) if mode == ADJACENT else 0)
    nl = names if isinstance(names, list) else names_list(names)
    assert names_list(parse.read_names) == [nl[int(w_order[int(w_group_off[g])])] for g in np.flatnonzero(w_kept)]


# ---------------------------------------------------------------------------------------------------------------------
# the fixture: 20 000 reads, 5 % extra unmapped records
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    st = synth.make_store(20_000, 500, seed=411)
    return synth.make_records(st, seed=412)


@pytest.fixture(scope="module")
def inputs(base):
    """(style, shuffled) -> (records, names, secondary), made once"""
    cache = {}

    def get(style, shuffled):
        if (style, shuffled) not in cache:
            cache[style, shuffled] = synth.make_named_records(base, style=style, seed=413, unmapped_rate=0.05, shuffle=shuffled)
        return cache[style, shuffled]
    return get


def test_the_fixture_is_what_the_tests_need(base, inputs):
    rec, names, sec = inputs("uuid", False)
    store, kept, dt, parse = DeviceStore.from_named_records(base.filters, base.txp_len, rec, names, secondary=sec)
    with store:
        assert parse.n_unmapped > 0.05 * len(base.records) and parse.n_unmapped + parse.n_parsed == len(rec)
        assert dt["no_mapping"] < base.discard["no_mapping"]              # the unmapped-only reads are no groups at all
        assert dt["no_mapping"] == 0 and parse.n_groups == len(base.group_off) - 1 - base.discard["no_mapping"]
        assert np.count_nonzero(kept) > 0.9 * parse.n_groups and store.n_reads == 20_000 == parse.n_reads


# ---------------------------------------------------------------------------------------------------------------------
# 1. equals the hand join
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,style,with_sec,model,coding,layout_build", [
    (ADJACENT, "uuid", True, -1, 0, 0), (SORT, "uuid", True, -1, 0, 0), (ADJACENT, "illumina", False, 0, 0, 0),
    (SORT, "illumina", False, 1, 0, 0), (SORT, "uuid", False, 0, 2, 0), (ADJACENT, "uuid", True, 1, 1, 1),
    (SORT, "illumina", True, -1, 1, 1), (ADJACENT, "illumina", False, -1, 2, 0), (SORT, "uuid", True, 0, 0, 1)])
def test_one_call_equals_the_hand_join(base, inputs, mode, style, with_sec, model, coding, layout_build):
    rec, names, sec = inputs(style, mode == SORT)
    sec = sec if with_sec else None
    kw = dict(weight_coding=coding, layout_build=layout_build)
    want = hand_join(base.filters, base.txp_len, rec, names, sec, mode, COVERAGE[model], **kw)
    one, kept, dt, parse = DeviceStore.from_named_records(base.filters, base.txp_len, rec, names, secondary=sec, mode=MODES[mode],
                                                          coverage=COVERAGE[model], **kw)
    with one, want[0] as long:
        check_outputs(parse, kept, dt, want, names, len(rec), mode, 100_000)
        assert one.n_reads == np.count_nonzero(kept) > 15_000       # (a permuted read's records come back primary first, then by index)
        if mode == ADJACENT:
            assert one.n_reads == 20_000
        rows = [n.decode() for n in names_list(parse.read_names)]
        _compare(one, long, len(base.txp_len), COVERAGE[model], rows)


# ---------------------------------------------------------------------------------------------------------------------
# 2. edge shapes of the new kernels
# ---------------------------------------------------------------------------------------------------------------------
def simple_records(n, unmapped):
    rec = np.zeros(n, dtype=ALN_RECORD)
    i = np.arange(n)
    rec["ref_id"], rec["aln_start"], rec["aln_end"], rec["aln_span"] = i % T, 10, 1500, 1400
    rec["score"], rec["seq_len"], rec["flags"] = 1000 - (i % 3), 1500, _lib.REC_HAS_SCORE
    rec["flags"][np.asarray(unmapped, dtype=bool)] = UNMAPPED
    rec["ref_id"][np.asarray(unmapped, dtype=bool)] = 0xFFFFFFFF
    return rec


def host_walk(L, rec, names, sec, mode, check):
    blob, off = names
    n = len(rec)
    order, goff, info = np.zeros(max(n, 1), np.uint32), np.zeros(n + 1, np.uint64), np.zeros(7, np.uint64)
    if not len(blob):
        blob = np.zeros(1, dtype=np.uint8)
    rc = L.oem_test_parse_bulk_host(rec.ctypes.data if n else None, n, blob.ctypes.data if n else None, off.ctypes.data,
                                    None if sec is None or not n else sec.ctypes.data, mode, check, order.ctypes.data, goff.ctypes.data,
                                    info.ctypes.data)
    u, p, g, c = (int(x) for x in info[:4])
    return rc, dict(order=order[:p].tolist(), group_off=goff[:g + 1].tolist(), n_unmapped=u, n_parsed=p, n_groups=g, n_checked=c), \
        tuple(int(x) for x in info[4:])


def run_case(L, unm, names, sec, mode, check, join=True):
    """One input through the device, held to the host walk and (join) to the hand join; returns the parse and the last-call record."""
    tl = np.full(T, 2000, dtype=np.uint64)
    rec = simple_records(len(names), unm)
    packed = pack(names)
    sec = None if sec is None else np.asarray(sec, dtype=np.uint8)
    rc, walk, _ = host_walk(L, rec, packed, sec, mode, check)
    assert rc == _lib.OEM_OK
    store, kept, dt, parse = DeviceStore.from_named_records(FILTERS, tl, rec, packed, secondary=sec, mode=MODES[mode], sort_check_num=check)
    last = (C.c_double * 8)()
    L.oem_debug_records_names_last_call(last)
    with store:
        got = dict(order=parse.order.tolist(), group_off=parse.group_off.tolist(), n_unmapped=parse.n_unmapped, n_parsed=parse.n_parsed,
                   n_groups=parse.n_groups, n_checked=parse.n_checked)
        assert got == walk
        if join:
            want = hand_join(FILTERS, tl, rec, packed, sec, mode)
            with want[0] as long:
                check_outputs(parse, kept, dt, want, list(names), len(rec), mode, check)
                assert (store.n_reads, store.nnz) == (long.n_reads, long.nnz)
    return parse, list(last)


def placements(n):
    out = {"nowhere": np.zeros(n, bool), "everywhere": np.ones(n, bool)}
    for name, at in (("first", [0]), ("last", [n - 1]), ("run across 256", list(range(250, 262)))):
        m = np.zeros(n, bool)
        m[[i for i in at if 0 <= i < n]] = True
        out[name] = m
    return out


@pytest.mark.parametrize("n", [0, 1, 51, 52, 255, 256, 257, 513])
def test_edge_shapes(n):
    """the gather's five words per record meet its 256 lanes at 51 / 52 records; the scans' and kernels' workgroups at 256"""
    rng = np.random.default_rng(n)
    reads = np.repeat(np.arange(n), rng.integers(1, 4, size=max(n, 1)))[:n]
    names = [b"read-%05d" % r for r in reads]
    sec = (np.arange(n) % 2).astype(np.uint8)
    with _lib.testing() as L:
        for where, unm in placements(n).items():
            for mode in (ADJACENT, SORT):
                if mode == SORT:
                    perm = np.random.default_rng(n + 1).permutation(n)
                    parse, last = run_case(L, unm, [names[i] for i in perm], sec, mode, 100_000)
                else:
                    parse, last = run_case(L, unm, names, sec, mode, 100_000)
                if where in ("nowhere",) and n:
                    assert last[1] == 0                                           # no name was gathered: the blob where it is
                    if mode == ADJACENT:
                        assert parse.order.tolist() == list(range(n)) and last[0] == 0    # the identity, and no record moved
                    else:
                        assert last[0] == 1
                elif n and 0 < parse.n_parsed < n:
                    assert last[0] == 1 and last[1] == 1
                assert last[3] == 0


def test_one_byte_names_and_names_across_the_gather_workgroups_blob_boundary():
    with _lib.testing() as L:
        # one-byte names: 255 of them, runs of two, with unmapped records so that the names are gathered (no check: they repeat)
        n = 513
        names = [bytes([1 + (i // 2) % 255]) for i in range(n)]
        unm = (np.arange(n) % 7 == 3)
        for mode in (ADJACENT, SORT):
            parse, last = run_case(L, unm, names, None, mode, 0)
            assert last[1] == 1 and parse.n_groups >= 255
        # 300-byte names: every 2 KiB of the gathered blob ends inside a name
        long_names = [(b"%04d" % (i // 2)) * 75 for i in range(52)]
        unm = (np.arange(52) % 5 == 0)
        for mode in (ADJACENT, SORT):
            parse, last = run_case(L, unm, long_names, None, mode, 100_000)
            assert last[1] == 1 and len(parse.read_names[0]) == 300 * parse.n_reads > 2048


@pytest.mark.parametrize("part", range(4))
def test_the_parse_cases_on_the_device(part):
    """every case of tests/test_parse_names.py through the device: the host walk's order, group_off and info, the
    oracle's verdict of the collation check with its group and both records"""
    tl = np.full(T, 2000, dtype=np.uint64)
    cases = list(parse_cases().items())[part::4]
    n_repeat = 0
    with _lib.testing() as L:
        for name, (unm, names, sec, mode, check) in cases:
            try:
                oracle(unm, names, sec, mode, check)
            except NotCollated as e:
                n_repeat += 1
                rec, packed = simple_records(len(names), unm), pack(names)
                s8 = None if sec is None else np.asarray(sec, dtype=np.uint8)
                rc, _, rep = host_walk(L, rec, packed, s8, mode, check)
                assert rc == _lib.OEM_ERR_STATE and rep == (e.group, e.record, e.earlier), name
                with pytest.raises(oarfish_amd.OemError) as ei:
                    DeviceStore.from_named_records(FILTERS, tl, rec, packed, secondary=s8, mode=MODES[mode], sort_check_num=check)
                msg = str(ei.value)
                assert ei.value.code == _lib.OEM_ERR_STATE, (name, msg)
                assert f"group {e.group} (first record {e.record})" in msg and f"(first record {e.earlier})" in msg, (name, msg)
                assert "OEM_COLLATE_SORT" in msg and NAME in msg
                continue
            run_case(L, unm, names, sec, mode, check, join=name.startswith("random") is False or int(name.split()[1]) % 5 == 0)
    assert n_repeat >= 1


# ---------------------------------------------------------------------------------------------------------------------
# 3. the collation check at scale
# ---------------------------------------------------------------------------------------------------------------------
def test_coordinate_sorted_like_input_is_refused_and_sort_accepts_it(base, inputs):
    rec, names, sec = inputs("uuid", False)
    nl = names_list(names)
    n = len(rec)
    mapped = (rec["flags"] & UNMAPPED) == 0
    # every read's records in two distant blocks: its first surviving record, then (after all reads' firsts) the others
    first = np.zeros(n, bool)
    prev = None
    for i in np.flatnonzero(mapped):
        if nl[i] != prev:
            first[i] = True
        prev = nl[i]
    split = np.concatenate([np.flatnonzero(first | ~mapped), np.flatnonzero(~first & mapped)])
    rec2, names2, sec2 = rec[split], gather_names(names, split), sec[split]
    nl2 = [nl[i] for i in split]
    G_a = int(first.sum())
    with pytest.raises(NotCollated) as oe:
        oracle(~mapped[split], nl2, None, ADJACENT, 100_000)
    assert oe.value.group == G_a and G_a < 100_000
    args = (base.filters, base.txp_len, rec2, names2)
    with pytest.raises(oarfish_amd.OemError) as ei:
        DeviceStore.from_named_records(*args, secondary=sec2)
    msg = str(ei.value)
    assert ei.value.code == _lib.OEM_ERR_STATE and "OEM_COLLATE_SORT" in msg
    assert f"group {G_a} (first record {oe.value.record})" in msg and f"(first record {oe.value.earlier})" in msg
    with pytest.raises(oarfish_amd.OemError):
        DeviceStore.from_named_records(*args, secondary=sec2, sort_check_num=G_a + 1)
    # a repeat at group N passes, and so does no check at all: the split reads are two rows each, as the reference's would be
    for check in (G_a, 0):
        want = hand_join(*args, sec2, ADJACENT)
        store, kept, dt, parse = DeviceStore.from_named_records(*args, secondary=sec2, sort_check_num=check)
        with store, want[0]:
            check_outputs(parse, kept, dt, want, nl2, n, ADJACENT, check)
            assert parse.n_groups > G_a and store.n_reads > 20_000
    # the same input under SORT: the collated input's store, read by read
    collated, kept_c, dt_c, parse_c = DeviceStore.from_named_records(base.filters, base.txp_len, rec, names, secondary=sec)
    store, kept, dt, parse = DeviceStore.from_named_records(*args, secondary=sec2, mode="sort")
    with collated, store:
        by_name_c = dict(zip(names_list(parse_c.read_names), kept_c[kept_c > 0].tolist()))
        by_name = dict(zip(names_list(parse.read_names), kept[kept > 0].tolist()))
        assert by_name == by_name_c and dt == dt_c and len(by_name) == 20_000
        assert (parse.n_groups, parse.unique_alignments) == (parse_c.n_groups, parse_c.unique_alignments)
        ca, ia = store.em_run()
        cb, ib = collated.em_run()
        floor = 1e-5 * store.n_reads / store.n_txps
        print("niter", ia.niter, ib.niter, "worst rel", float(np.max(np.abs(ca - cb) / np.maximum(np.abs(cb), floor))))
        assert ia.niter == ib.niter
        assert_counts_close(ca, cb, store.n_reads, store.n_txps, rtol=1e-10, what="sorted against collated")


# ---------------------------------------------------------------------------------------------------------------------
# 4. errors found on the device
# ---------------------------------------------------------------------------------------------------------------------
def _good_call():
    tl = np.full(T, 2000, dtype=np.uint64)
    names = [b"read-%03d" % (i // 2) for i in range(40)]
    store, kept, _, parse = DeviceStore.from_named_records(FILTERS, tl, simple_records(40, np.zeros(40, bool)), pack(names))
    with store:
        assert store.n_reads == 20 == parse.n_reads and kept.tolist() == [2] * 20


def test_a_bad_name_is_named_by_its_input_index_unless_its_record_is_unmapped():
    tl = np.full(T, 2000, dtype=np.uint64)
    for unm, names, at, zero in bad_name_cases():
        for mode in (ADJACENT, SORT):
            for extra_unmapped in (False, True):       # without and with unmapped records: the blob in place, the gathered blob
                u = np.array(unm, bool)
                if not extra_unmapped and u.any():
                    continue
                if extra_unmapped:
                    u = u.copy()
                    u[[i for i in (2, 21, 38) if i != at]] = True
                with pytest.raises(oarfish_amd.OemError) as ei:
                    DeviceStore.from_named_records(FILTERS, tl, simple_records(40, u), pack(names), mode=MODES[mode])
                msg = str(ei.value)
                assert ei.value.code == _lib.OEM_ERR_ARG and NAME in msg
                assert (f"the name of record {at} contains a 0 byte" if zero else f"record {at} has an empty name") in msg, (at, zero, msg)
                _good_call()
        u = np.array(unm, bool)                        # the same bad name on an unmapped record is accepted
        u[at] = True
        if at == 17:
            u[30] = True
        store, _, _, parse = DeviceStore.from_named_records(FILTERS, tl, simple_records(40, u), pack(names), sort_check_num=0)
        with store:
            assert parse.n_unmapped == int(u.sum()) and store.n_reads > 0


def test_a_ref_id_that_is_no_transcript_and_an_alignment_outside_its_transcript():
    tl = np.full(T, 2000, dtype=np.uint64)
    names = [b"read-%03d" % (i // 2) for i in range(300)]
    unm = np.arange(300) % 11 == 5
    for mode in (ADJACENT, SORT):
        rec = simple_records(300, unm)
        rec["ref_id"][[201, 260]] = [T, T + 3]                                         # a later one is not the one named (ADJACENT)
        perm = np.random.default_rng(3).permutation(300) if mode == SORT else np.arange(300)
        with pytest.raises(oarfish_amd.OemError) as ei:
            DeviceStore.from_named_records(FILTERS, tl, rec[perm], pack([names[i] for i in perm]), mode=MODES[mode])
        msg = str(ei.value)
        assert ei.value.code == _lib.OEM_ERR_ARG and NAME in msg and "is not below n_txps" in msg
        at = int(np.flatnonzero(perm == 201)[0])
        assert f"record {at}: ref_id {T} " in msg, msg
        _good_call()
        rec = simple_records(300, unm)
        rec["aln_end"][100] = 2600                                                     # past its transcript's 2000
        with pytest.raises(oarfish_amd.OemError) as ei:
            DeviceStore.from_named_records(FILTERS, tl, rec[perm], pack([names[i] for i in perm]), mode=MODES[mode], coverage="logistic")
        assert ei.value.code == _lib.OEM_ERR_STATE and "outside its transcript" in str(ei.value)
        store, _, _, _ = DeviceStore.from_named_records(FILTERS, tl, rec[perm], pack([names[i] for i in perm]), mode=MODES[mode])
        store.close()                                                                  # without a coverage model the store exists
        _good_call()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the host loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [ADJACENT, SORT])
def test_scores_beyond_2_to_24_and_a_zero_denominator_take_the_host_loop(mode):
    tl = np.full(T, 2000, dtype=np.uint64)
    n = 600
    names = [b"read-%03d" % (i // 2) for i in range(n)]
    unm = np.arange(n) % 13 == 4
    rec = simple_records(n, unm)
    sec = (np.arange(n) % 2).astype(np.uint8)
    perm = np.random.default_rng(8).permutation(n) if mode == SORT else np.arange(n)
    big = rec.copy()
    big["score"][[300, 301]] = [2 ** 24 + 1, 2 ** 24 - 3]
    with _lib.testing() as L:
        last = (C.c_double * 8)()
        for F, r in ((FILTERS, big), (dict(FILTERS, score_prob_denom=0.0), rec)):
            args = (F, tl, r[perm], pack([names[i] for i in perm]))
            want = hand_join(*args, sec[perm], mode)
            store, kept, dt, parse = DeviceStore.from_named_records(*args, secondary=sec[perm], mode=MODES[mode])
            L.oem_debug_records_names_last_call(last)
            assert last[3] == 1                                                        # the host loop took the groups
            with store, want[0] as long:
                check_outputs(parse, kept, dt, want, [names[i] for i in perm], n, mode, 100_000)
                assert (store.n_reads, store.nnz) == (long.n_reads, long.nnz) and store.n_reads > 250
                for a, b in zip(store.aux_counts(), long.aux_counts()):
                    assert np.array_equal(a, b)
        store, _, _, _ = DeviceStore.from_named_records(FILTERS, tl, rec[perm], pack([names[i] for i in perm]), mode=MODES[mode])
        L.oem_debug_records_names_last_call(last)
        store.close()
        assert last[3] == 0                                                            # without the planted scores: the device


# ---------------------------------------------------------------------------------------------------------------------
# 6. outputs that are NULL
# ---------------------------------------------------------------------------------------------------------------------
def test_every_optional_output_may_be_null(base, inputs):
    rec, (blob, off), sec = inputs("illumina", True)
    F = filters_c(base.filters)
    tl = np.ascontiguousarray(base.txp_len, dtype=np.uint64)
    L = _lib.lib()
    h = C.c_void_p()
    rc = L.oem_store_create_records_names(C.addressof(F), tl.ctypes.data, len(tl), rec.ctypes.data, len(rec), blob.ctypes.data, off.ctypes.data,
                                          sec.ctypes.data, SORT, 100_000, 100, -1, 2.0, 0, None, None, None, None, None, None, None, None,
                                          C.byref(h))
    assert rc == _lib.OEM_OK, L.oem_last_error()
    bare = DeviceStore._adopt(L, h, len(tl), 0)
    full, _, _, parse = DeviceStore.from_named_records(base.filters, tl, rec, (blob, off), secondary=sec, mode="sort")
    with bare, full:
        _compare(bare, full, len(tl), None, [n.decode() for n in names_list(parse.read_names)])


# ---------------------------------------------------------------------------------------------------------------------
# 7. the bulk driver
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True])
def test_the_bulk_driver_from_records(base, inputs, on_device, tmp_path):
    from oarfish_amd.bulk import BulkArgs, perform_inference_and_write_output, quantify_bulk_alignments_from_records
    rec, names, sec = inputs("uuid", False)
    T_ = len(base.txp_len)
    txps = [f"ENST{i:011d}.{i % 13}" for i in range(T_)]
    lens = [int(x) for x in base.txp_len]
    out = str(tmp_path / "one" / "sample")
    args = BulkArgs(output=out, write_assignment_probs=True, display_thresh=1e-4, prob_on_device=on_device, quant_on_device=on_device)
    got = quantify_bulk_alignments_from_records(base.filters, txps, lens, rec, names, args, secondary=sec)

    # the hand join's host store, and perform_inference_and_write_output on it with the hand join's read names
    idx = np.flatnonzero((rec["flags"] & UNMAPPED) == 0)
    nl = names_list(names)
    order, group_off, _ = oarfish_amd.collate_names(gather_names(names, idx), [0, len(idx)], mode="adjacent")
    with StoreBuilder(base.filters, base.txp_len) as hb:
        kept = hb.add_groups(rec[idx][order], group_off)
        row_ptr, tid, p = hb.export()[:3]
    rnames = [nl[int(idx[order[int(group_off[g])]])].decode() for g in np.flatnonzero(kept)]
    host = InMemoryAlignmentStore.from_arrays(row_ptr, tid, p)
    ref_out = str(tmp_path / "ref" / "sample")
    ref = perform_inference_and_write_output(host, txps, lens, BulkArgs(output=ref_out, write_assignment_probs=True, display_thresh=1e-4),
                                             read_names=rnames)
    assert_counts_close(got, ref, len(rnames), T_, rtol=1e-10, what="the driver from records against the driver on the host store")

    # the same counts into both sides: the files byte for byte
    dev = host.device_store(T_, 0)
    want_out = str(tmp_path / "want" / "sample")
    writers.write_output(want_out, {}, txps, lens, got, *dev.aux_counts())
    writers.write_out_prob(want_out, row_ptr, tid, dev.assignment_probs(got, 1e-4), rnames, txps, 1e-4)
    for ext in (".quant", ".ambig_info.tsv", ".prob"):
        assert open(out + ext, "rb").read() == open(want_out + ext, "rb").read(), ext
    name_col = lambda path: [ln.split(b"\t")[0] for ln in open(path, "rb").read().split(b"\n")[T_ + 1:]]   # noqa: E731
    assert name_col(out + ".prob") == name_col(ref_out + ".prob") and len(name_col(out + ".prob")) == 20_000 + 1
    assert open(out + ".ambig_info.tsv", "rb").read() == open(ref_out + ".ambig_info.tsv", "rb").read()
    if np.array_equal(got, ref):
        for ext in (".quant", ".prob", ".meta_info.json"):
            a, b = open(out + ext, "rb").read(), open(ref_out + ext, "rb").read()
            assert a == b.replace(ref_out.encode(), out.encode()), ext
    host.invalidate_device()
