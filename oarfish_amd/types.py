"""Host-side mirror of the reference types the EM path consumes.

Reference (COMBINE-lab/oarfish v0.10.3, src/util/oarfish_types.rs):
  ``InMemoryAlignmentStore``  :548-558, iter :651-656, len :562-564,
                              add_filtered_group :718-738, total_len / num_aligned_reads :741-748
  ``TranscriptInfo``          :431-437 (only ``len``/``lenf`` reach the EM, and only with the KDE)
  ``EMInfo``                  :408-428
  ``AlignmentFilters.model_coverage`` :792 (selects whether cov_prob is used, em.rs:108)

Same names and argument meaning as the reference so the parity tests read like
its own would; the arrays are NumPy, and the HBM-resident form is created lazily
by :meth:`InMemoryAlignmentStore.device_store`.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Iterator, Optional, Sequence, Tuple

import numpy as np

from . import _lib


@dataclass
class AlignmentFilters:
    """Only the field the EM reads (oarfish_types.rs:792)."""
    model_coverage: bool = False


@dataclass
class TranscriptInfo:
    """oarfish_types.rs:431-437.  The EM reads ``lenf`` only under --use-kde."""
    len: int = 1
    total_weight: float = 0.0
    lenf: float = 1.0

    @classmethod
    def with_len(cls, length: int) -> "TranscriptInfo":
        return cls(len=int(length), total_weight=0.0, lenf=float(length))


@dataclass
class RunInfo:
    """What do_em / em_par leave behind besides the counts (oem_run_info)."""
    niter: int
    n_passes: int
    converged: bool
    rel_diff: float


class AssignmentText:
    """What ``DeviceStore.assignment_text`` returns: ``text``, the body lines of the `.prob` file as one contiguous
    ``uint8`` array (a bytes-like buffer: ``fh.write(r.text)``, ``bytes(r.text)``); ``line_off``, the ``n_reads + 1``
    byte offsets of the lines; ``kept``, the ``k`` of each line.  From ``DeviceStore.assignment_text_lz4`` ``text`` is
    the LZ4 frame of the whole file instead (``line_off`` still describes the uncompressed body), and the result also
    carries ``content_bytes``, ``n_blocks`` and ``raw_blocks``."""

    def __init__(self, text: np.ndarray, line_off: np.ndarray, kept: np.ndarray):
        self.text = text
        self.line_off = line_off
        self.kept = kept

    def __len__(self) -> int:
        return len(self.kept)

    def line(self, r: int) -> bytes:
        return self.text[int(self.line_off[r]):int(self.line_off[r + 1])].tobytes()


def take_text_result(L, h, offsets: bool = True) -> AssignmentText:
    """The ``AssignmentText`` of an ``oem_text_result`` handle of a call that needs no store (oem_count_matrix_text,
    oem_quant_text, oem_ambig_text), which is released.  ``offsets=False`` leaves ``line_off`` and ``kept`` ``None``
    (a writer needs the text alone)."""
    try:
        nb, nl = C.c_uint64(0), C.c_uint64(0)
        _lib.check(L.oem_text_result_dims(h, C.byref(nb), C.byref(nl), None))
        text = np.empty(nb.value, dtype=np.uint8)
        line_off = np.empty(nl.value + 1, dtype=np.uint64) if offsets else None
        kept = np.empty(nl.value, dtype=np.uint32) if offsets else None
        _lib.check(L.oem_text_result_copy(h, text.ctypes.data if nb.value else None,
                                          line_off.ctypes.data if offsets else None,
                                          kept.ctypes.data if offsets and nl.value else None))
        res = AssignmentText(text, line_off, kept)
        res.content_bytes = int(nb.value)
    finally:
        L.oem_text_result_destroy(h)
    return res


def pack_read_names(read_names, n_reads: int):
    """Read names as the C ABI takes them: (blob uint8, offsets uint64[n_reads + 1]).  ``read_names`` is a sequence of
    ``str`` / ``bytes`` or already such a pair."""
    if isinstance(read_names, tuple) and len(read_names) == 2 and not isinstance(read_names[1], (str, bytes)):
        blob = np.ascontiguousarray(np.frombuffer(read_names[0], dtype=np.uint8) if isinstance(read_names[0], (bytes, bytearray, memoryview))
                                    else read_names[0], dtype=np.uint8)
        off = np.ascontiguousarray(read_names[1], dtype=np.uint64)
        if len(off) != n_reads + 1 or int(off[-1]) > len(blob):
            raise ValueError("read_names offsets must have n_reads + 1 entries that end inside the blob")
        return blob, off
    enc = [n.encode("utf-8") if isinstance(n, str) else bytes(n) for n in read_names]
    if len(enc) != n_reads:
        raise ValueError("read_names length != n_reads")
    off = np.zeros(n_reads + 1, dtype=np.uint64)
    np.cumsum(np.fromiter(map(len, enc), dtype=np.uint64, count=n_reads), out=off[1:])
    return np.frombuffer(b"".join(enc), dtype=np.uint8), off


class DeviceStore:
    """RAII wrapper of an ``oem_store*`` (the matrix resident in HBM on one GPU)."""

    def __init__(self, row_ptr, tid, as_prob, cov_prob, n_txps: int, device: int = 0,
                 reorder_rows: int = 0, window_cap: int = 0, layout_build: int = 0, weight_coding: int = 0):
        self._h = C.c_void_p()
        self.row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
        tid = np.ascontiguousarray(tid, dtype=np.uint32)
        as_prob = np.ascontiguousarray(as_prob, dtype=np.float32)
        cov = None if cov_prob is None else np.ascontiguousarray(cov_prob, dtype=np.float64)
        self.n_reads = len(self.row_ptr) - 1
        self.nnz = len(tid)
        self.n_txps = int(n_txps)
        self.device = int(device)
        if len(as_prob) != self.nnz or (cov is not None and len(cov) != self.nnz):
            raise ValueError("tid / as_prob / cov_prob lengths differ")
        opts = _lib.StoreOptsC()
        opts.reorder_rows = reorder_rows
        opts.window_cap = window_cap      # 0 = chosen from the store; 512 / 2048 force it (oem_store_opts)
        opts.layout_build = layout_build  # 1 = host layout builder (the specification)
        opts.weight_coding = weight_coding  # 1 = never dictionary-code the local weights
        L = _lib.lib()
        self._lib = L                     # the library that owns the handle
        self._check(L.oem_store_create(
            self.row_ptr.ctypes.data, tid.ctypes.data if self.nnz else None,
            as_prob.ctypes.data if self.nnz else None,
            None if cov is None else cov.ctypes.data, self.n_reads, self.nnz, self.n_txps,
            self.device, C.addressof(opts), C.byref(self._h)))

    @classmethod
    def with_coverage(cls, row_ptr, tid, as_prob, aln_start, aln_end, txp_len, bin_width: int = 100,
                      model: str = "logistic", growth_rate: float = 2.0, device: int = 0, reorder_rows: int = 0,
                      window_cap: int = 0, layout_build: int = 0, weight_coding: int = 0,
                      return_coverage: bool = False):
        """The bulk coverage model and the store on its column in one device call (oem_store_create_coverage):
        the store ``DeviceStore(row_ptr, tid, as_prob, cov, len(txp_len), ...)`` would be, where ``cov`` is the
        column of ``oem_coverage_probs_device`` (logistic with ``growth_rate``, or binomial) on the alignments'
        ``aln_start`` / ``aln_end``; the column and the weights never leave the device.  With ``return_coverage``
        returns ``(store, cov)`` (nnz f64, NaN for a zero-span alignment, whose read the EM drops)."""
        models = {"logistic": 0, "binomial": 1}
        if model not in models:
            raise ValueError(f"model must be one of {sorted(models)}, not {model!r}")
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        self.row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
        tid = np.ascontiguousarray(tid, dtype=np.uint32)
        as_prob = np.ascontiguousarray(as_prob, dtype=np.float32)
        aln_start = np.ascontiguousarray(aln_start, dtype=np.uint32)
        aln_end = np.ascontiguousarray(aln_end, dtype=np.uint32)
        txp_len = np.ascontiguousarray(txp_len, dtype=np.uint64)
        self.n_reads = len(self.row_ptr) - 1
        self.nnz = len(tid)
        self.n_txps = len(txp_len)
        self.device = int(device)
        if len(as_prob) != self.nnz or len(aln_start) != self.nnz or len(aln_end) != self.nnz:
            raise ValueError("tid, as_prob, aln_start and aln_end must have one entry per alignment")
        opts = _lib.StoreOptsC()
        opts.reorder_rows = reorder_rows
        opts.window_cap = window_cap
        opts.layout_build = layout_build
        opts.weight_coding = weight_coding  # 2: the products rounded once to f32 (oem_store_opts)
        cov = np.empty(self.nnz, dtype=np.float64) if return_coverage else None
        nz = self.nnz > 0
        L = _lib.lib()
        self._lib = L
        self._check(L.oem_store_create_coverage(
            self.row_ptr.ctypes.data, tid.ctypes.data if nz else None, as_prob.ctypes.data if nz else None,
            aln_start.ctypes.data if nz else None, aln_end.ctypes.data if nz else None, txp_len.ctypes.data,
            self.n_reads, self.nnz, self.n_txps, bin_width, models[model], growth_rate, self.device,
            C.addressof(opts), cov.ctypes.data if cov is not None and nz else None, C.byref(self._h)))
        return (self, cov) if return_coverage else self

    @classmethod
    def _adopt(cls, L, handle, n_txps: int, device: int) -> "DeviceStore":
        """A DeviceStore around a handle the library has just returned (the CSR has no host copy: ``row_ptr`` is None)."""
        self = cls.__new__(cls)
        self._h = handle
        self._lib = L
        self.row_ptr = None
        self.n_txps = int(n_txps)
        self.device = int(device)
        R, nnz, T = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        self._check(L.oem_store_dims(handle, C.byref(R), C.byref(nnz), C.byref(T)))
        self.n_reads, self.nnz = int(R.value), int(nnz.value)
        return self

    @classmethod
    def from_records(cls, filters, txp_len, records, group_off, coverage: Optional[str] = None, bin_width: int = 100,
                     growth_rate: float = 2.0, device: int = 0, reorder_rows: int = 0, window_cap: int = 0,
                     layout_build: int = 0, weight_coding: int = 0):
        """Alignment records -> resident store in one device call (oem_store_create_records): the filter cascade of
        AlignmentFilters::filter runs on the GPU and the CSR never exists on the host.  ``records`` / ``group_off`` as in
        ``builder.StoreBuilder.add_groups``; ``coverage``: None, "logistic" or "binomial".  Returns
        ``(store, kept, discard_table)``: ``kept[g]`` alignments of group g were kept, read r of the store is the r-th
        group with ``kept > 0`` (pick the read names for ``assignment_text`` with it), and the discard table is a dict
        with DiscardTable's counters.  The store is the one ``StoreBuilder(...).add_groups(...)`` followed by
        ``device_store(coverage, ...)`` gives."""
        from . import builder as _b
        fc = _b.filters_c(filters)
        txp_len = np.ascontiguousarray(txp_len, dtype=np.uint64)
        records, group_off = _b.check_batch(records, group_off)
        n_groups = len(group_off) - 1
        kept = np.zeros(n_groups, dtype=np.uint32)
        dt = _lib.DiscardTableC()
        o = _b.store_opts(reorder_rows, window_cap, layout_build, weight_coding)
        L = _lib.lib()
        h = C.c_void_p()
        rc = L.oem_store_create_records(C.addressof(fc), txp_len.ctypes.data, len(txp_len),
                                        records.ctypes.data if len(records) else None, group_off.ctypes.data, n_groups,
                                        bin_width, _b._model_code(coverage), growth_rate, int(device), C.addressof(o),
                                        kept.ctypes.data, C.addressof(dt), C.byref(h))
        if rc != _lib.OEM_OK:
            msg = L.oem_last_error()
            raise _lib.OemError(rc, msg.decode("utf-8", "replace") if msg else "")
        return cls._adopt(L, h, len(txp_len), device), kept, _b.discard_dict(dt)

    @classmethod
    def from_named_records(cls, filters, txp_len, records, names, secondary=None, mode: str = "adjacent",
                           sort_check_num: int = 100_000, coverage: Optional[str] = None, bin_width: int = 100,
                           growth_rate: float = 2.0, device: int = 0, reorder_rows: int = 0, window_cap: int = 0,
                           layout_build: int = 0, weight_coding: int = 0):
        """Records and read names in input order -> resident store in one device call (oem_store_create_records_names):
        the reference's bulk parser (alignment_parser.rs:301-437) and ``from_records`` joined on the GPU.  Unmapped
        records are skipped before the reads are cut; ``mode="adjacent"`` is the reference's parser (name-collated input,
        refused with OEM_ERR_STATE when one of the first ``sort_check_num`` reads repeats an earlier name; 0 = no check),
        ``mode="sort"`` collates input in any order by read name on the device.  ``names``: one per record, a sequence of
        ``str`` / ``bytes`` or a ``(blob, offsets)`` pair; ``secondary``: one flag per record, or None.

        Returns ``(store, kept, discard_table, parse)``: the first three as ``from_records`` returns them for the groups
        of the parsed input; ``parse`` has ``order`` (input indices of the surviving records, collated), ``group_off``
        (positions of ``order`` where a read starts, then ``n_parsed``), ``read_names`` (the names of the store's rows as
        a ``(blob, offsets)`` pair, what ``assignment_text`` and ``writers.write_out_prob_device`` take as is),
        ``n_unmapped``, ``n_parsed``, ``n_groups``, ``n_reads``, ``unique_alignments`` and ``n_checked``."""
        from types import SimpleNamespace

        from . import builder as _b
        modes = {"sort": _lib.OEM_COLLATE_SORT, "adjacent": _lib.OEM_COLLATE_ADJACENT}
        if mode not in modes:
            raise ValueError(f"mode must be one of {sorted(modes)}, not {mode!r}")
        fc = _b.filters_c(filters)
        txp_len = np.ascontiguousarray(txp_len, dtype=np.uint64)
        records = np.ascontiguousarray(records, dtype=_b.ALN_RECORD)
        n = len(records)
        packed = isinstance(names, tuple) and len(names) == 2 and not isinstance(names[1], (str, bytes))
        if (len(names[1]) - 1 if packed else len(names)) != n:
            raise ValueError("names must have one entry per record")
        blob, off = pack_read_names(names, n)
        sec = None
        if secondary is not None:
            sec = np.ascontiguousarray(np.asarray(secondary) != 0, dtype=np.uint8)
            if len(sec) != n:
                raise ValueError("secondary must have one entry per record")
        if n and not len(blob):
            blob = np.zeros(1, dtype=np.uint8)   # (every name is empty: the call says so)
        order = np.empty(max(n, 1), dtype=np.uint32)
        group_off = np.empty(n + 1, dtype=np.uint64)
        kept = np.empty(max(n, 1), dtype=np.uint32)
        row_blob = np.empty(max(int(off[n]), 1), dtype=np.uint8)
        row_off = np.empty(n + 1, dtype=np.uint64)
        dt, pi = _lib.DiscardTableC(), _lib.ParseInfoC()
        o = _b.store_opts(reorder_rows, window_cap, layout_build, weight_coding)
        L = _lib.lib()
        h = C.c_void_p()
        rc = L.oem_store_create_records_names(C.addressof(fc), txp_len.ctypes.data, len(txp_len), records.ctypes.data if n else None, n,
                                              blob.ctypes.data if n else None, off.ctypes.data,
                                              None if sec is None or not n else sec.ctypes.data, modes[mode], int(sort_check_num),
                                              bin_width, _b._model_code(coverage), growth_rate, int(device), C.addressof(o),
                                              order.ctypes.data, group_off.ctypes.data, kept.ctypes.data, row_blob.ctypes.data,
                                              row_off.ctypes.data, C.addressof(dt), C.addressof(pi), C.byref(h))
        if rc != _lib.OEM_OK:
            msg = L.oem_last_error()
            raise _lib.OemError(rc, msg.decode("utf-8", "replace") if msg else "")
        row_off = row_off[:pi.n_reads + 1].copy()
        parse = SimpleNamespace(order=order[:pi.n_parsed].copy(), group_off=group_off[:pi.n_groups + 1].copy(),
                                read_names=(row_blob[:int(row_off[-1])].copy(), row_off), n_unmapped=int(pi.n_unmapped),
                                n_parsed=int(pi.n_parsed), n_groups=int(pi.n_groups), n_reads=int(pi.n_reads),
                                unique_alignments=int(pi.unique_alignments), n_checked=int(pi.n_checked))
        return cls._adopt(L, h, len(txp_len), device), kept[:pi.n_groups].copy(), _b.discard_dict(dt), parse

    @classmethod
    def from_projected_records(cls, filters, txp_len, records, group_off, read_len, beta: float = 10.0,
                               prob_source="similarity", coverage: Optional[str] = None, bin_width: int = 100,
                               growth_rate: float = 2.0, device: int = 0, reorder_rows: int = 0, window_cap: int = 0,
                               layout_build: int = 0, weight_coding: int = 0):
        """Projected (genome-mode) records -> resident store in one device call (oem_store_create_projected_records):
        AlignmentFilters::filter_projected runs on the GPU.  ``records`` / ``group_off`` / ``read_len`` / ``beta`` /
        ``prob_source`` as in ``builder.StoreBuilder.add_projected_groups``, the rest and the returned
        ``(store, kept, discard_table)`` as in ``from_records``.  The store is the one
        ``StoreBuilder(...).add_projected_groups(...)`` followed by ``device_store(coverage, ...)`` gives."""
        from . import builder as _b
        fc = _b.filters_c(filters)
        txp_len = np.ascontiguousarray(txp_len, dtype=np.uint64)
        records, group_off, read_len = _b.check_projected_batch(records, group_off, read_len)
        po = _b.proj_opts_c(beta, prob_source)
        n_groups = len(group_off) - 1
        kept = np.zeros(n_groups, dtype=np.uint32)
        dt = _lib.DiscardTableC()
        o = _b.store_opts(reorder_rows, window_cap, layout_build, weight_coding)
        L = _lib.lib()
        h = C.c_void_p()
        rc = L.oem_store_create_projected_records(C.addressof(fc), txp_len.ctypes.data, len(txp_len),
                                                  records.ctypes.data if len(records) else None, group_off.ctypes.data,
                                                  read_len.ctypes.data if n_groups else None, n_groups, C.addressof(po),
                                                  bin_width, _b._model_code(coverage), growth_rate, int(device),
                                                  C.addressof(o), kept.ctypes.data, C.addressof(dt), C.byref(h))
        if rc != _lib.OEM_OK:
            msg = L.oem_last_error()
            raise _lib.OemError(rc, msg.decode("utf-8", "replace") if msg else "")
        return cls._adopt(L, h, len(txp_len), device), kept, _b.discard_dict(dt)

    def _check(self, rc: int) -> None:
        if rc != _lib.OEM_OK:
            msg = self._lib.oem_last_error()
            raise _lib.OemError(rc, msg.decode("utf-8", "replace") if msg else "")

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.oem_store_destroy(self._h)
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
            raise RuntimeError("DeviceStore is closed")
        return self._h

    # -- queries ----------------------------------------------------------
    def bytes(self) -> Tuple[int, int]:
        hbm, alg = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.oem_store_bytes(self.handle, C.byref(hbm), C.byref(alg)))
        return int(hbm.value), int(alg.value)

    def set_option(self, option: int, value: int):
        self._check(self._lib.oem_store_set_option(self.handle, option, value))

    # -- compute ----------------------------------------------------------
    def m_step(self, theta, row_w=None) -> np.ndarray:
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if len(theta) != self.n_txps:
            raise ValueError("theta length != n_txps")
        out = np.zeros(self.n_txps, dtype=np.float64)
        wp = None
        if row_w is not None:
            row_w = np.ascontiguousarray(row_w, dtype=np.uint32)
            if len(row_w) != self.n_reads:
                raise ValueError("row_w length != n_reads")
            wp = row_w.ctypes.data
        self._check(self._lib.oem_m_step(self.handle, theta.ctypes.data, wp, out.ctypes.data))
        return out

    def em_run(self, init=None, max_iter=1000, conv_thresh=1e-3, min_iter_gate=50):
        out = np.zeros(self.n_txps, dtype=np.float64)
        ri = _lib.RunInfoC()
        ip = None
        if init is not None:
            init = np.ascontiguousarray(init, dtype=np.float64)
            if len(init) != self.n_txps:
                raise ValueError("init_abundances length != n_txps")
            ip = init.ctypes.data
        self._check(self._lib.oem_em_run(self.handle, ip, max_iter, conv_thresh, min_iter_gate,
                                         out.ctypes.data, C.byref(ri)))
        return out, RunInfo(ri.niter, ri.n_passes, bool(ri.converged), ri.rel_diff)

    def run_history(self, run: int = 0) -> np.ndarray:
        """The rel_diff of every loop pass of run ``run`` of the last ``em_run`` (run 0) or ``bootstrap``
        (replicate ``run``) on this store, recorded on the device under
        ``set_option(_lib.OEM_OPT_RUN_HISTORY, K)`` (oem_run_history): entry ``k`` is the value the stopping rule
        saw at ``niter == k``, so the reference's line ``iteration N; rel diff R`` is entry ``N - 1``, and the last
        entry is ``RunInfo.rel_diff``.  At most ``min(K, max_iter)`` entries are stored; ``run_history_len`` gives
        the run's full count.  Raises ``OemError`` (OEM_ERR_STATE) when the last call recorded nothing."""
        n = min(self.run_history_len(run), self.info(_lib.OEM_INFO_RUN_HISTORY_STORED))  # what was stored
        out = np.zeros(n, dtype=np.float64)
        self._check(self._lib.oem_run_history(self.handle, run, out.ctypes.data if n else None, n, None))
        return out

    def run_history_len(self, run: int = 0) -> int:
        """``niter + converged`` of that run: its loop passes, recorded or not."""
        n = C.c_uint32(0)
        self._check(self._lib.oem_run_history(self.handle, run, None, 0, C.byref(n)))
        return int(n.value)

    def aux_counts(self):
        """aux_counts.rs:23-50 -> (unique_count u32[T], total_count u32[T])."""
        u = np.zeros(self.n_txps, dtype=np.uint32)
        t = np.zeros(self.n_txps, dtype=np.uint32)
        self._check(self._lib.oem_aux_counts(self.handle, u.ctypes.data, t.ctypes.data))
        return u, t

    def assignment_probs(self, counts, display_thresh: float) -> np.ndarray:
        """write_function.rs:283-318: per-alignment printed probability, -1 where omitted."""
        counts = np.ascontiguousarray(counts, dtype=np.float64)
        if len(counts) != self.n_txps:
            raise ValueError("counts length != n_txps")
        out = np.zeros(self.nnz, dtype=np.float64)
        self._check(self._lib.oem_assignment_probs(self.handle, counts.ctypes.data, display_thresh,
                                                   out.ctypes.data))
        return out

    def assignment_text(self, counts, display_thresh: float, read_names=None) -> AssignmentText:
        """write_function.rs:283-332: the body lines of the `.prob` file, formatted on the device
        (oem_assignment_text) -- byte for byte what ``writers.write_out_prob`` writes after its header lines from
        ``assignment_probs``, except that a read whose kept probabilities are all 0/0 prints them as Rust's ``NaN``.  ``read_names``: a sequence of ``str`` /
        ``bytes``, a pair ``(blob, offsets)``, or None (every name empty)."""
        counts = np.ascontiguousarray(counts, dtype=np.float64)
        if len(counts) != self.n_txps:
            raise ValueError("counts length != n_txps")
        blob = off = None
        if read_names is not None:
            blob, off = pack_read_names(read_names, self.n_reads)
            if len(blob) == 0:
                blob = np.zeros(1, dtype=np.uint8)     # a non-NULL pointer: the names exist, they are all empty
        L = self._lib
        h = C.c_void_p()
        self._check(L.oem_assignment_text(self.handle, counts.ctypes.data, display_thresh,
                                          None if blob is None else blob.ctypes.data,
                                          None if off is None else off.ctypes.data, C.byref(h)))
        try:
            nb, nl, nk = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
            self._check(L.oem_text_result_dims(h, C.byref(nb), C.byref(nl), C.byref(nk)))
            text = np.empty(nb.value, dtype=np.uint8)
            line_off = np.empty(nl.value + 1, dtype=np.uint64)
            kept = np.empty(nl.value, dtype=np.uint32)
            self._check(L.oem_text_result_copy(h, text.ctypes.data if nb.value else None, line_off.ctypes.data,
                                               kept.ctypes.data if nl.value else None))
        finally:
            L.oem_text_result_destroy(h)
        return AssignmentText(text, line_off, kept)

    def assignment_text_lz4(self, counts, display_thresh: float, read_names=None, prefix: bytes = b"") -> AssignmentText:
        """The `.prob.lz4` file (write_function.rs:243-263, 334-337) compressed on the device
        (oem_assignment_text_lz4): ``text`` is one complete LZ4 frame whose content is ``prefix`` -- the file's header
        lines -- followed by exactly the bytes ``assignment_text`` returns for the same arguments; ``line_off`` and
        ``kept`` are that call's (offsets into the body, after the prefix).  The result also has ``content_bytes``
        (prefix + body), ``n_blocks`` and ``raw_blocks`` (blocks stored uncompressed)."""
        counts = np.ascontiguousarray(counts, dtype=np.float64)
        if len(counts) != self.n_txps:
            raise ValueError("counts length != n_txps")
        blob = off = None
        if read_names is not None:
            blob, off = pack_read_names(read_names, self.n_reads)
            if len(blob) == 0:
                blob = np.zeros(1, dtype=np.uint8)     # a non-NULL pointer: the names exist, they are all empty
        pre = np.frombuffer(bytes(prefix), dtype=np.uint8)
        L = self._lib
        h = C.c_void_p()
        self._check(L.oem_assignment_text_lz4(self.handle, counts.ctypes.data, display_thresh,
                                              None if blob is None else blob.ctypes.data,
                                              None if off is None else off.ctypes.data,
                                              pre.ctypes.data if len(pre) else None, len(pre), C.byref(h)))
        try:
            nb, nl, nk = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
            self._check(L.oem_text_result_dims(h, C.byref(nb), C.byref(nl), C.byref(nk)))
            text = np.empty(nb.value, dtype=np.uint8)
            line_off = np.empty(nl.value + 1, dtype=np.uint64)
            kept = np.empty(nl.value, dtype=np.uint32)
            self._check(L.oem_text_result_copy(h, text.ctypes.data, line_off.ctypes.data,
                                               kept.ctypes.data if nl.value else None))
            res = AssignmentText(text, line_off, kept)
            v = C.c_uint64(0)
            for name, key in (("content_bytes", _lib.OEM_TEXT_INFO_CONTENT_BYTES), ("n_blocks", _lib.OEM_TEXT_INFO_BLOCKS),
                              ("raw_blocks", _lib.OEM_TEXT_INFO_RAW_BLOCKS)):
                self._check(L.oem_text_result_info(h, key, C.byref(v)))
                setattr(res, name, int(v.value))
        finally:
            L.oem_text_result_destroy(h)
        return res

    def bootstrap_weights(self, seed: int, replica: int) -> np.ndarray:
        w = np.zeros(self.n_reads, dtype=np.uint32)
        self._check(self._lib.oem_bootstrap_weights(self.handle, seed, replica, w.ctypes.data))
        return w

    def bootstrap(self, n_boot: int, seed: int = 0, row_w_all=None, init=None, max_iter=1000,
                  conv_thresh=1e-3, first_replica: int = 0):
        """n_boot replicates; replicate k uses the device resample of global replica
        ``first_replica + k`` (a pure function of (seed, replica), so processes holding the same
        store can split one set of replicates)."""
        self.set_option(_lib.OEM_OPT_BOOTSTRAP_FIRST_REPLICA, int(first_replica))
        out = np.zeros((n_boot, self.n_txps), dtype=np.float64)
        infos = (_lib.RunInfoC * max(n_boot, 1))()
        wp = None
        if row_w_all is not None:
            row_w_all = np.ascontiguousarray(row_w_all, dtype=np.uint32)
            if row_w_all.shape != (n_boot, self.n_reads):
                raise ValueError("row_w_all must be n_boot x n_reads")
            wp = row_w_all.ctypes.data
        ip = None
        if init is not None:
            init = np.ascontiguousarray(init, dtype=np.float64)
            if len(init) != self.n_txps:
                raise ValueError("init_abundances length != n_txps")
            ip = init.ctypes.data
        self._check(self._lib.oem_bootstrap(self.handle, n_boot, seed, wp, ip, max_iter, conv_thresh,
                                            out.ctypes.data, C.addressof(infos)))
        return out, [RunInfo(i.niter, i.n_passes, bool(i.converged), i.rel_diff)
                     for i in list(infos)[:n_boot]]

    def time_m_step(self, n_launches: int) -> float:
        ms = C.c_float(0)
        self._check(self._lib.oem_time_m_step(self.handle, n_launches, C.byref(ms)))
        return float(ms.value)

    def info(self, key: int) -> int:
        """oem_store_info: _lib.OEM_INFO_WEIGHT_DICT_ENTRIES / _TILES / _REMOTE_ALIGNMENTS / _RUN_HISTORY_STORED."""
        v = C.c_uint64(0)
        self._check(self._lib.oem_store_info(self.handle, key, C.byref(v)))
        return int(v.value)

    def time_em_iters(self, n_iters: int) -> float:
        ms = C.c_float(0)
        self._check(self._lib.oem_time_em_iters(self.handle, n_iters, C.byref(ms)))
        return float(ms.value)

    def time_bootstrap_passes(self, n_passes: int):
        """(ms per batched bootstrap pass, replicates per pass, algorithmic bytes per batched pass)."""
        ms, slots, nbytes = C.c_float(0), C.c_uint32(0), C.c_uint64(0)
        self._check(self._lib.oem_time_bootstrap_passes(self.handle, n_passes, C.byref(ms), C.byref(slots),
                                                        C.byref(nbytes)))
        return float(ms.value), int(slots.value), int(nbytes.value)

    def time_allreduce(self, n_calls: int) -> float:
        """Collective: microseconds per all-reduce of the n_txps count vector (the exchange by itself)."""
        us = C.c_float(0)
        self._check(self._lib.oem_time_allreduce(self.handle, n_calls, C.byref(us)))
        return float(us.value)

    def attach_comm(self, comm_handle, global_n_reads: int, global_row_offset: int):
        self._check(self._lib.oem_store_attach_comm(self.handle, comm_handle, global_n_reads,
                                                    global_row_offset))


class InMemoryAlignmentStore:
    """oarfish_types.rs:548-558: per-read groups of (ref_id, as_prob f32, cov_prob f64).

    ``alignments`` holds ref_id only (the one AlnInfo field the EM reads,
    em.rs:41,60,103,120); ``boundaries`` is the row-pointer array that is
    private in the reference (:555).
    """

    def __init__(self, filter_opts: Optional[AlignmentFilters] = None):
        self.filter_opts = filter_opts or AlignmentFilters()
        self._chunks_tid = []
        self._chunks_p = []
        self._lens = []
        self.alignments = np.zeros(0, dtype=np.uint32)          # ref_id per alignment
        self.as_probabilities = np.zeros(0, dtype=np.float32)
        self.coverage_probabilities = np.zeros(0, dtype=np.float64)
        self.boundaries = np.zeros(1, dtype=np.uint64)          # oarfish_types.rs:645
        self._dirty = False
        self._dev = {}

    # -- construction -------------------------------------------------------
    @classmethod
    def from_arrays(cls, boundaries, ref_ids, as_probabilities, coverage_probabilities=None,
                    model_coverage: Optional[bool] = None) -> "InMemoryAlignmentStore":
        st = cls(AlignmentFilters(model_coverage=bool(
            coverage_probabilities is not None if model_coverage is None else model_coverage)))
        st.boundaries = np.ascontiguousarray(boundaries, dtype=np.uint64)
        st.alignments = np.ascontiguousarray(ref_ids, dtype=np.uint32)
        st.as_probabilities = np.ascontiguousarray(as_probabilities, dtype=np.float32)
        if coverage_probabilities is None:
            # add_filtered_group fills zeros (oarfish_types.rs:731-732)
            st.coverage_probabilities = np.zeros(len(st.alignments), dtype=np.float64)
        else:
            st.coverage_probabilities = np.ascontiguousarray(coverage_probabilities, dtype=np.float64)
        if st.boundaries[0] != 0 or st.boundaries[-1] != len(st.alignments):
            raise ValueError("boundaries must start at 0 and end at the number of alignments")
        return st

    def add_filtered_group(self, ref_ids: Sequence[int], as_probs: Sequence[float]) -> bool:
        """oarfish_types.rs:718-738: append one read's retained alignments; empty groups are dropped."""
        if len(ref_ids) == 0:
            return False
        if len(ref_ids) != len(as_probs):
            raise ValueError("ref_ids and as_probs differ in length")
        self._chunks_tid.append(np.asarray(ref_ids, dtype=np.uint32))
        self._chunks_p.append(np.asarray(as_probs, dtype=np.float32))
        self._lens.append(len(ref_ids))
        self._dirty = True
        return True

    def _flush(self):
        if not self._dirty:
            return
        self.alignments = np.concatenate([self.alignments] + self._chunks_tid)
        self.as_probabilities = np.concatenate([self.as_probabilities] + self._chunks_p)
        new_b = int(self.boundaries[-1]) + np.cumsum(np.asarray(self._lens, dtype=np.uint64))
        self.boundaries = np.concatenate([self.boundaries, new_b.astype(np.uint64)])
        self.coverage_probabilities = np.concatenate(
            [self.coverage_probabilities,
             np.zeros(len(self.alignments) - len(self.coverage_probabilities), dtype=np.float64)])
        self._chunks_tid, self._chunks_p, self._lens = [], [], []
        self._dirty = False
        self.invalidate_device()

    # -- reference accessors ------------------------------------------------
    def len(self) -> int:                       # oarfish_types.rs:562-564
        self._flush()
        return len(self.boundaries) - 1

    __len__ = len

    def num_aligned_reads(self) -> int:         # :746-748
        return self.len()

    def total_len(self) -> int:                 # :741-743
        self._flush()
        return len(self.alignments)

    def iter(self) -> Iterator[Tuple[np.ndarray, np.ndarray, np.ndarray]]:  # :651-656
        self._flush()
        b = self.boundaries
        for i in range(len(b) - 1):
            s, e = int(b[i]), int(b[i + 1])
            yield self.alignments[s:e], self.as_probabilities[s:e], self.coverage_probabilities[s:e]

    __iter__ = iter

    # -- HBM-resident form ----------------------------------------------------
    def invalidate_device(self):
        for _stamp, d in self._dev.values():
            d.close()
        self._dev = {}

    def model_coverage_on_device(self, aln_start, aln_end, txp_len, bin_width: int = 100, growth_rate: float = 2.0,
                                 device: int = 0, weight_coding: int = 0) -> np.ndarray:
        """bulk.rs:103-108 on the device: ``filter_opts.model_coverage`` on, the logistic coverage model of the
        alignments (``aln_start`` / ``aln_end`` per alignment, ``txp_len`` per transcript) normalised per read into
        ``coverage_probabilities``, where the reference's store holds it after ``normalize_read_probs``.  The store is
        created on the device in the same call (``DeviceStore.with_coverage``) and kept as this store's resident
        copy for ``len(txp_len)`` transcripts: ``em``, ``em_par``, ``bootstrap``, ``aux_counts`` and
        ``assignment_probs`` then run on it without a second upload.  ``weight_coding`` 2 keeps the weights as f32
        (oem_store_opts).  Returns the column."""
        self._flush()
        n_txps = len(txp_len)
        dev, cov = DeviceStore.with_coverage(self.boundaries, self.alignments, self.as_probabilities, aln_start,
                                             aln_end, txp_len, bin_width=bin_width, model="logistic",
                                             growth_rate=growth_rate, device=device, weight_coding=weight_coding,
                                             return_coverage=True)
        self.filter_opts.model_coverage = True
        self.coverage_probabilities = cov
        key = (int(device), int(n_txps))
        old = self._dev.pop(key, None)
        if old is not None:
            old[1].close()
        self._dev[key] = (self._stamp(cov), dev)
        return cov

    def _stamp(self, cov):
        return (self.boundaries, self.alignments, self.as_probabilities, cov, bool(self.filter_opts.model_coverage))

    def device_store(self, n_txps: int, device: int = 0) -> DeviceStore:
        """Upload once, keep resident (the analogue of the store living in RAM across
        em / bootstrap calls, bulk.rs:131-194)."""
        self._flush()
        cov = self.coverage_probabilities if self.filter_opts.model_coverage else None  # em.rs:108
        # The reference mutates the store between calls (normalize_read_probs fills
        # coverage_probabilities, bulk.rs:103-108): the resident copy is keyed by the identity of the
        # arrays it was made from and by model_coverage, and re-made when any of them is replaced.
        # (In-place writes into an array after its upload need an explicit invalidate_device().)
        key = (int(device), int(n_txps))
        # the stamp holds the arrays themselves (compared with `is`): an id() alone can be reused by a
        # later array once the first one is freed, and a stale resident copy would then look current
        stamp = self._stamp(cov)
        hit = self._dev.get(key)
        if hit is not None and not (len(hit[0]) == len(stamp) and
                                    all(a is b for a, b in zip(hit[0][:4], stamp[:4])) and hit[0][4] == stamp[4]):
            hit[1].close()
            hit = None
        if hit is None:
            hit = (stamp, DeviceStore(self.boundaries, self.alignments, self.as_probabilities, cov, n_txps, device))
            self._dev[key] = hit
        return hit[1]


@dataclass
class EMInfo:
    """oarfish_types.rs:408-428."""
    eq_map: InMemoryAlignmentStore
    txp_info: Sequence[TranscriptInfo]
    max_iter: int = 1000                 # prog_opts.rs:532
    convergence_thresh: float = 1e-3     # prog_opts.rs:536
    init_abundances: Optional[np.ndarray] = None
    kde_model: Optional[object] = None   # hidden --use-kde: not supported (SURVEY.md 8a note 4)
    device: int = 0
    last_run_info: Optional[RunInfo] = field(default=None, compare=False)
    last_run_history: Optional[np.ndarray] = field(default=None, compare=False)  # em / em_par: rel_diff per loop pass
