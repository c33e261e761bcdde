"""The store builder: alignment records -> the CSR the EM consumes.

``StoreBuilder`` wraps ``oem_builder_*``: AlignmentFilters::filter + add_filtered_group
(src/util/oarfish_types.rs:955-1130, :718-738) per read, one read per call (``add_group``) or a batch of reads per call
(``add_groups``), on the host or -- ``device=`` -- on the GPU (oem_filter_device.hip), with the same builder state
afterwards byte for byte.  ``DeviceStore.from_records`` (types.py) goes from the records to a resident store in one
call, without the CSR ever existing on the host.

Records are a numpy structured array of dtype ``ALN_RECORD`` (the 40 bytes of ``oem_aln_record``); group g of a batch
is ``records[group_off[g]:group_off[g + 1]]``.

Genome mode has its own pair: ``add_projected_group`` / ``add_projected_groups`` run AlignmentFilters::filter_projected
(:1179-1297) over records of dtype ``PROJ_RECORD`` (``oem_proj_record``) with one read length per group, into the same
builder; ``DeviceStore.from_projected_records`` is the one-call form.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from ._lib import REC_HAS_SCORE, REC_REVERSE, REC_SUPPLEMENTARY, REC_UNMAPPED  # noqa: F401  (re-exported)

ALN_RECORD = np.dtype([("ref_id", "<u4"), ("aln_start", "<u4"), ("aln_end", "<u4"), ("aln_span", "<u4"),
                       ("score", "<i8"), ("seq_len", "<i8"), ("flags", "<u4"), ("reserved", "<u4")])
assert ALN_RECORD.itemsize == C.sizeof(_lib.AlnRecordC) == 40

PROJ_RECORD = np.dtype([("similarity", "<f8"), ("ref_id", "<u4"), ("start", "<u4"), ("end", "<u4"), ("aligned_len", "<u4"),
                        ("query_aligned_len", "<u4"), ("aln_score", "<i4"), ("flags", "<u4"), ("reserved", "<u4")])
assert PROJ_RECORD.itemsize == C.sizeof(_lib.ProjRecordC) == 40
PROB_SOURCES = {"similarity": _lib.PROJ_SIMILARITY, "score": _lib.PROJ_SCORE, "combined": _lib.PROJ_COMBINED}

DISCARD_FIELDS = tuple(n for n, _ in _lib.DiscardTableC._fields_)


def filters_c(filters) -> _lib.FiltersC:
    """An ``oem_filters`` from a ``FiltersC``, a mapping or any object with the fields of AlignmentFilters
    (five_prime_clip, three_prime_clip, score_threshold, min_aligned_fraction, min_aligned_len, which_strand,
    score_prob_denom)."""
    if isinstance(filters, _lib.FiltersC):
        return filters
    get = (lambda k: filters[k]) if isinstance(filters, dict) else (lambda k: getattr(filters, k))
    return _lib.FiltersC(int(get("five_prime_clip")), int(get("three_prime_clip")), float(get("score_threshold")),
                         float(get("min_aligned_fraction")), int(get("min_aligned_len")), int(get("which_strand")),
                         float(get("score_prob_denom")), 0)


def check_batch(records, group_off):
    """(records, group_off) as the contiguous arrays the C calls read."""
    records = np.ascontiguousarray(records, dtype=ALN_RECORD)
    group_off = np.ascontiguousarray(group_off, dtype=np.uint64)
    if group_off.ndim != 1 or len(group_off) < 1:
        raise ValueError("group_off needs n_groups + 1 entries")
    if int(group_off[-1]) > len(records):
        raise ValueError("group_off runs past the end of records")
    return records, group_off


def proj_opts_c(beta: float = 10.0, prob_source="similarity") -> _lib.ProjOptsC:
    """An ``oem_proj_opts``: ``prob_source`` by name ("similarity", "score", "combined") or by its code."""
    if isinstance(prob_source, str):
        if prob_source not in PROB_SOURCES:
            raise ValueError(f"prob_source must be one of {sorted(PROB_SOURCES)}, not {prob_source!r}")
        prob_source = PROB_SOURCES[prob_source]
    return _lib.ProjOptsC(float(beta), int(prob_source))


def check_projected_batch(records, group_off, read_len):
    """(records, group_off, read_len) as the contiguous arrays the projected batch calls read."""
    records = np.ascontiguousarray(records, dtype=PROJ_RECORD)
    group_off = np.ascontiguousarray(group_off, dtype=np.uint64)
    read_len = np.ascontiguousarray(read_len, dtype=np.uint64)
    if group_off.ndim != 1 or len(group_off) < 1:
        raise ValueError("group_off needs n_groups + 1 entries")
    if int(group_off[-1]) > len(records):
        raise ValueError("group_off runs past the end of records")
    if read_len.shape != (len(group_off) - 1,):
        raise ValueError("read_len needs n_groups entries")
    return records, group_off, read_len


def discard_dict(dt: _lib.DiscardTableC) -> dict:
    return {n: int(getattr(dt, n)) for n in DISCARD_FIELDS}


class StoreBuilder:
    """RAII wrapper of an ``oem_builder*``."""

    def __init__(self, filters, txp_len):
        self._lib = _lib.lib()
        self.filters = filters_c(filters)
        self.txp_len = np.ascontiguousarray(txp_len, dtype=np.uint64)
        self._h = C.c_void_p()
        self._check(self._lib.oem_builder_create(C.addressof(self.filters), self.txp_len.ctypes.data, len(self.txp_len),
                                                 C.byref(self._h)))

    def _check(self, rc: int) -> None:
        if rc != _lib.OEM_OK:
            msg = self._lib.oem_last_error()
            raise _lib.OemError(rc, msg.decode("utf-8", "replace") if msg else "")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.oem_builder_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        if not self._h.value:
            raise RuntimeError("StoreBuilder is closed")
        return self._h

    # -- filling -----------------------------------------------------------------------------------------------------
    def add_group(self, records) -> int:
        """One read's records; returns the number of alignments kept (0: the read was dropped)."""
        records = np.ascontiguousarray(records, dtype=ALN_RECORD)
        kept = C.c_uint32(0)
        self._check(self._lib.oem_builder_add_group(self.handle, records.ctypes.data if len(records) else None,
                                                    len(records), C.byref(kept)))
        return int(kept.value)

    def add_groups(self, records, group_off, device: Optional[int] = None) -> np.ndarray:
        """A batch of reads in one call, on the host (``device=None``) or on GPU ``device``.  Returns ``kept`` (u32 per
        group: what ``add_group`` would have returned); row r of what the call appends is the r-th group with
        ``kept > 0``.  The call is atomic: on an error the builder is unchanged."""
        records, group_off = check_batch(records, group_off)
        n_groups = len(group_off) - 1
        kept = np.zeros(n_groups, dtype=np.uint32)
        rec = records.ctypes.data if len(records) else None
        if device is None:
            rc = self._lib.oem_builder_add_groups(self.handle, rec, group_off.ctypes.data, n_groups, kept.ctypes.data)
        else:
            rc = self._lib.oem_builder_add_groups_device(self.handle, rec, group_off.ctypes.data, n_groups, int(device),
                                                         kept.ctypes.data)
        self._check(rc)
        return kept

    def add_projected_group(self, records, read_len: int, beta: float = 10.0, prob_source="similarity") -> int:
        """One genome-mode read's projected records (dtype ``PROJ_RECORD``) through filter_projected
        (oarfish_types.rs:1179-1297); returns the number of alignments kept (0: the read was dropped)."""
        records = np.ascontiguousarray(records, dtype=PROJ_RECORD)
        po = proj_opts_c(beta, prob_source)
        kept = C.c_uint32(0)
        self._check(self._lib.oem_builder_add_projected_group(self.handle, records.ctypes.data if len(records) else None,
                                                              len(records), int(read_len), C.addressof(po), C.byref(kept)))
        return int(kept.value)

    def add_projected_groups(self, records, group_off, read_len, beta: float = 10.0, prob_source="similarity",
                             device: Optional[int] = None) -> np.ndarray:
        """A batch of genome-mode reads in one call, as ``add_groups``: ``read_len[g]`` is read g's length,
        ``prob_source`` "similarity", "score" or "combined" (ProjProbSource), ``beta`` --projected-prob-beta.  On the
        host (``device=None``) or on GPU ``device``, with the same builder state afterwards byte for byte.  Atomic."""
        records, group_off, read_len = check_projected_batch(records, group_off, read_len)
        po = proj_opts_c(beta, prob_source)
        n_groups = len(group_off) - 1
        kept = np.zeros(n_groups, dtype=np.uint32)
        rec = records.ctypes.data if len(records) else None
        rl = read_len.ctypes.data if n_groups else None
        if device is None:
            rc = self._lib.oem_builder_add_projected_groups(self.handle, rec, group_off.ctypes.data, rl, n_groups,
                                                            C.addressof(po), kept.ctypes.data)
        else:
            rc = self._lib.oem_builder_add_projected_groups_device(self.handle, rec, group_off.ctypes.data, rl, n_groups,
                                                                   C.addressof(po), int(device), kept.ctypes.data)
        self._check(rc)
        return kept

    # -- reading -----------------------------------------------------------------------------------------------------
    def dims(self):
        """(n_reads, nnz)"""
        R, nnz = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.oem_builder_dims(self.handle, C.byref(R), C.byref(nnz)))
        return int(R.value), int(nnz.value)

    def export(self):
        """(row_ptr u64, tid u32, as_prob f32, start u32, end u32, strand u8)"""
        R, nnz = self.dims()
        rp = np.zeros(R + 1, dtype=np.uint64)
        tid, p = np.zeros(nnz, dtype=np.uint32), np.zeros(nnz, dtype=np.float32)
        s, e, sd = np.zeros(nnz, dtype=np.uint32), np.zeros(nnz, dtype=np.uint32), np.zeros(nnz, dtype=np.uint8)
        self._check(self._lib.oem_builder_export(self.handle, rp.ctypes.data, tid.ctypes.data, p.ctypes.data,
                                                 s.ctypes.data, e.ctypes.data, sd.ctypes.data))
        return rp, tid, p, s, e, sd

    def discard_table(self) -> dict:
        dt = _lib.DiscardTableC()
        self._check(self._lib.oem_builder_discard_table(self.handle, C.addressof(dt)))
        return discard_dict(dt)

    # -- coverage model ------------------------------------------------------------------------------------------------
    def coverage_probs(self, bin_width: int = 100, growth_rate: float = 2.0) -> np.ndarray:
        out = np.zeros(self.dims()[1], dtype=np.float64)
        self._check(self._lib.oem_builder_coverage_probs(self.handle, bin_width, growth_rate, out.ctypes.data))
        return out

    def coverage_probs_binomial(self, bin_width: int = 100) -> np.ndarray:
        out = np.zeros(self.dims()[1], dtype=np.float64)
        self._check(self._lib.oem_builder_coverage_probs_binomial(self.handle, bin_width, out.ctypes.data))
        return out

    def coverage_probs_device(self, bin_width: int = 100, model: str = "logistic", growth_rate: float = 2.0,
                              device: int = 0) -> np.ndarray:
        out = np.zeros(self.dims()[1], dtype=np.float64)
        self._check(self._lib.oem_builder_coverage_probs_device(self.handle, bin_width, _model_code(model), growth_rate,
                                                                int(device), out.ctypes.data))
        return out

    # -- upload --------------------------------------------------------------------------------------------------------
    def device_store(self, coverage: Optional[str] = None, bin_width: int = 100, growth_rate: float = 2.0,
                     device: int = 0, cov_prob=None, **opts):
        """The built store on GPU ``device``: ``coverage=None`` -- oem_builder_store_create (with ``cov_prob``, a
        column computed elsewhere); "logistic" / "binomial" -- oem_builder_store_create_coverage.  ``opts``:
        reorder_rows, window_cap, layout_build, weight_coding (oem_store_opts)."""
        from .types import DeviceStore
        o = store_opts(**opts)
        h = C.c_void_p()
        if coverage is None:
            cov = None if cov_prob is None else np.ascontiguousarray(cov_prob, dtype=np.float64)
            self._check(self._lib.oem_builder_store_create(self.handle, None if cov is None else cov.ctypes.data,
                                                           int(device), C.addressof(o), C.byref(h)))
        else:
            self._check(self._lib.oem_builder_store_create_coverage(self.handle, bin_width, _model_code(coverage),
                                                                    growth_rate, int(device), C.addressof(o), None,
                                                                    C.byref(h)))
        return DeviceStore._adopt(self._lib, h, len(self.txp_len), int(device))


RECORDS_STREAM_INFO = {"batches": _lib.OEM_RECORDS_STREAM_INFO_BATCHES, "groups": _lib.OEM_RECORDS_STREAM_INFO_GROUPS,
                       "records": _lib.OEM_RECORDS_STREAM_INFO_RECORDS,
                       "batches_before_finish": _lib.OEM_RECORDS_STREAM_INFO_BATCHES_BEFORE_FINISH,
                       "blocked_us": _lib.OEM_RECORDS_STREAM_INFO_BLOCKED_US,
                       "host_batches": _lib.OEM_RECORDS_STREAM_INFO_HOST_BATCHES,
                       "row_name_bytes": _lib.OEM_RECORDS_STREAM_INFO_ROW_NAME_BYTES,
                       "host_finished": _lib.OEM_RECORDS_STREAM_INFO_HOST_FINISHED,
                       "arena_bytes": _lib.OEM_RECORDS_STREAM_INFO_ARENA_BYTES}


class RecordsStream:
    """The bulk records session (``oem_records_stream_*``): ``DeviceStore.from_records`` for a pipeline that never holds
    all records at once.  ``push`` batches of whole groups from any number of threads as they are parsed (each call
    copies its batch into page-locked staging and returns its ticket; the device filters batch k while batch k + 1 is
    staged); ``finish`` returns what ``from_records`` returns for the batches concatenated in ticket order.  A context
    manager: leaving the block destroys the session (an unfinished one is cancelled).

    ``names=True`` makes it a names session (``oem_records_stream_set_names``): ``push(records, names=...)`` takes
    records and their read names in input order, cut at any record positions (a read may straddle pushes), and ``finish``
    returns what ``DeviceStore.from_named_records(mode="adjacent", sort_check_num=...)`` returns for the concatenation.

    ``names=True, mode="sort"`` makes it a sorting names session (``oem_records_stream_set_sort``) for input in ANY
    order, a coordinate-sorted BAM for one: ``push(records, names=..., secondary=...)``, and ``finish`` returns what
    ``DeviceStore.from_named_records(secondary=..., mode="sort")`` returns for the concatenation, ``parse.order`` as
    ``int64`` session-global input indices.  The survivors stay on the device until ``finish``
    (``info()["arena_bytes"]``: the most the arena held): the session saves the run-sized host arrays, not device memory.

    ``projected=True`` makes it a projected session (``oem_records_stream_set_projected``) for genome mode:
    ``push(records, group_off, read_len=...)`` takes batches of whole groups of ``PROJ_RECORD`` with one read length per
    group, and ``finish`` returns what ``DeviceStore.from_projected_records(beta=..., prob_source=...)`` returns for the
    concatenation.  ``info()["host_finished"]`` is, after ``finish``, the number of alignments whose ``expf`` the host
    supplied."""

    def __init__(self, filters, txp_len, coverage: Optional[str] = None, bin_width: int = 100, growth_rate: float = 2.0,
                 device: int = 0, max_staged_records: int = 0, names: bool = False, sort_check_num: int = 100_000,
                 projected: bool = False, beta: float = 10.0, prob_source="similarity", mode: str = "adjacent"):
        if names and projected:
            raise ValueError("a session takes names=True or projected=True, not both")
        if mode not in ("adjacent", "sort"):
            raise ValueError(f"mode must be 'adjacent' or 'sort', not {mode!r}")
        if mode == "sort" and not names:
            raise ValueError('mode="sort" belongs to a names session (names=True)')
        po = proj_opts_c(beta, prob_source) if projected else None
        self._lib = _lib.lib()
        self.filters = filters_c(filters)
        self.txp_len = np.ascontiguousarray(txp_len, dtype=np.uint64)
        self.device = int(device)
        o = _lib.RecordsStreamOptsC()
        o.n_txps, o.device, o.bin_width, o.model = len(self.txp_len), self.device, bin_width, _model_code(coverage)
        o.growth_rate, o.max_staged_records = growth_rate, int(max_staged_records)
        self._h = C.c_void_p()
        self._check(self._lib.oem_records_stream_create(C.byref(o), C.addressof(self.filters), self.txp_len.ctypes.data,
                                                        C.byref(self._h)))
        self.names = bool(names)
        self.sorting = mode == "sort"
        if self.sorting:
            self._check(self._lib.oem_records_stream_set_sort(self._h))
        elif self.names:
            self._check(self._lib.oem_records_stream_set_names(self._h, int(sort_check_num)))
        self.projected = bool(projected)
        if self.projected:
            self._check(self._lib.oem_records_stream_set_projected(self._h, C.addressof(po)))

    _check = StoreBuilder._check

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.oem_records_stream_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        if not self._h.value:
            raise RuntimeError("RecordsStream is closed")
        return self._h

    def push(self, records, group_off=None, names=None, read_len=None, secondary=None) -> int:
        """One batch (``records`` / ``group_off`` as in ``StoreBuilder.add_groups``); returns its ticket.  Thread-safe;
        blocks while the staging budget is full.  A names session takes ``names=`` instead of ``group_off``: one name
        per record, a sequence of ``str`` / ``bytes`` or a ``(blob, offsets)`` pair, packed as ``from_named_records``
        packs it.  A projected session takes ``read_len=`` besides ``group_off``, as
        ``StoreBuilder.add_projected_groups`` does.  A sorting names session takes ``secondary=`` besides ``names=``:
        one flag per record, or None for a batch without secondary alignments."""
        if secondary is not None and not self.sorting:
            raise ValueError('secondary= belongs to a sorting names session (names=True, mode="sort")')
        if read_len is not None and not self.projected:
            raise ValueError("read_len= belongs to a projected session (projected=True)")
        if self.projected:
            if names is not None:
                raise ValueError("a projected session takes group_off and read_len=, not names=")
            if group_off is None or read_len is None:
                raise ValueError("a projected session's push needs group_off and read_len=")
            records, group_off, read_len = check_projected_batch(records, group_off, read_len)
            n_groups = len(group_off) - 1
            ticket = C.c_uint64(0)
            self._check(self._lib.oem_records_stream_push_projected(self.handle, records.ctypes.data if len(records) else None,
                                                                    group_off.ctypes.data, read_len.ctypes.data if n_groups else None,
                                                                    n_groups, C.byref(ticket)))
            return int(ticket.value)
        if names is not None:
            from .types import pack_read_names
            if group_off is not None:
                raise ValueError("push takes group_off or names, not both")
            records = np.ascontiguousarray(records, dtype=ALN_RECORD)
            n = len(records)
            packed = isinstance(names, tuple) and len(names) == 2 and not isinstance(names[1], (str, bytes))
            if (len(names[1]) - 1 if packed else len(names)) != n:
                raise ValueError("names must have one entry per record")
            blob, off = pack_read_names(names, n)
            if n and not len(blob):
                blob = np.zeros(1, dtype=np.uint8)   # (every name is empty: the session says so)
            ticket = C.c_uint64(0)
            if self.sorting:
                sec = None
                if secondary is not None:
                    sec = np.ascontiguousarray(np.asarray(secondary) != 0, dtype=np.uint8)
                    if len(sec) != n:
                        raise ValueError("secondary must have one entry per record")
                self._check(self._lib.oem_records_stream_push_sort(self.handle, records.ctypes.data if n else None, n,
                                                                   blob.ctypes.data if n else None, off.ctypes.data,
                                                                   None if sec is None or not n else sec.ctypes.data,
                                                                   C.byref(ticket)))
                return int(ticket.value)
            self._check(self._lib.oem_records_stream_push_names(self.handle, records.ctypes.data if n else None, n,
                                                                blob.ctypes.data if n else None, off.ctypes.data,
                                                                C.byref(ticket)))
            return int(ticket.value)
        if group_off is None:
            raise ValueError("push needs group_off (or names= on a names session)")
        records, group_off = check_batch(records, group_off)
        ticket = C.c_uint64(0)
        self._check(self._lib.oem_records_stream_push(self.handle, records.ctypes.data if len(records) else None,
                                                      group_off.ctypes.data, len(group_off) - 1, C.byref(ticket)))
        return int(ticket.value)

    def info(self) -> dict:
        out = {}
        for name, key in RECORDS_STREAM_INFO.items():
            if name == "row_name_bytes" and not self.names:   # (a names session's key)
                continue
            if name == "host_finished" and not self.projected:   # (a projected session's key)
                continue
            if name == "arena_bytes" and not self.sorting:   # (a sorting names session's key)
                continue
            v = C.c_uint64(0)
            self._check(self._lib.oem_records_stream_info(self.handle, key, C.byref(v)))
            out[name] = int(v.value)
        return out

    def finish(self, reorder_rows: int = 0, window_cap: int = 0, layout_build: int = 0, weight_coding: int = 0):
        """``(DeviceStore, kept, discard_table)`` as ``DeviceStore.from_records`` returns them for the accepted batches
        concatenated in ticket order.  A names session returns ``(DeviceStore, kept, discard_table, parse)`` as
        ``DeviceStore.from_named_records`` does, ``parse.order`` being None -- or, in a sorting names session, the
        collated survivors' session-global input indices as ``int64``."""
        from .types import DeviceStore
        o = store_opts(reorder_rows, window_cap, layout_build, weight_coding)
        if self.names:
            from types import SimpleNamespace
            dt, pi = _lib.DiscardTableC(), _lib.ParseInfoC()
            h = C.c_void_p()
            self._check(self._lib.oem_records_stream_finish_names(self.handle, C.addressof(o), C.addressof(dt), C.addressof(pi),
                                                                  C.byref(h)))
            store = DeviceStore._adopt(self._lib, h, len(self.txp_len), self.device)
            group_off = np.zeros(pi.n_groups + 1, dtype=np.uint64)
            kept = np.zeros(max(pi.n_groups, 1), dtype=np.uint32)
            row_blob = np.zeros(max(self.info()["row_name_bytes"], 1), dtype=np.uint8)
            row_off = np.zeros(pi.n_reads + 1, dtype=np.uint64)
            self._check(self._lib.oem_records_stream_names_copy(self.handle, group_off.ctypes.data, kept.ctypes.data,
                                                                row_blob.ctypes.data, row_off.ctypes.data))
            order = None
            if self.sorting:
                order = np.zeros(pi.n_parsed, dtype=np.int64)
                self._check(self._lib.oem_records_stream_order_copy(self.handle, order.ctypes.data if pi.n_parsed else None))
            parse = SimpleNamespace(order=order, group_off=group_off, read_names=(row_blob[:int(row_off[-1])].copy(), row_off),
                                    n_unmapped=int(pi.n_unmapped), n_parsed=int(pi.n_parsed), n_groups=int(pi.n_groups),
                                    n_reads=int(pi.n_reads), unique_alignments=int(pi.unique_alignments),
                                    n_checked=int(pi.n_checked))
            return store, kept[:pi.n_groups].copy(), discard_dict(dt), parse
        kept = np.zeros(self.info()["groups"], dtype=np.uint32)
        dt = _lib.DiscardTableC()
        h = C.c_void_p()
        self._check(self._lib.oem_records_stream_finish(self.handle, C.addressof(o), kept.ctypes.data, C.addressof(dt),
                                                        C.byref(h)))
        return DeviceStore._adopt(self._lib, h, len(self.txp_len), self.device), kept, discard_dict(dt)


def _model_code(model) -> int:
    codes = {None: -1, "logistic": 0, "binomial": 1}
    if model not in codes:
        raise ValueError(f"coverage model must be None, 'logistic' or 'binomial', not {model!r}")
    return codes[model]


def store_opts(reorder_rows: int = 0, window_cap: int = 0, layout_build: int = 0, weight_coding: int = 0) -> _lib.StoreOptsC:
    o = _lib.StoreOptsC()
    o.reorder_rows, o.window_cap, o.layout_build, o.weight_coding = reorder_rows, window_cap, layout_build, weight_coding
    return o
