"""Host-side mirror of the reference's EM interface, running on the MI355X engine.

Reference (COMBINE-lab/oarfish v0.10.3, src/em.rs):
  ``em(&EMInfo, nthreads) -> Vec<f64>``            :262-271   (gate niter>50, :212)
  ``em_par(&EMInfo, nthreads) -> Vec<f64>``        :320-447   (gate niter>1,  :399)
  ``bootstrap(&EMInfo, num_boot, nthreads) -> Vec<Vec<f64>>``  :292-314

Same names, argument meaning and results (un-normalised expected read counts,
em.rs:254).  ``nthreads`` is accepted and ignored, as ``em`` itself ignores it
(em.rs:262 ``_nthreads``); the work runs on the GPU that holds the store.
The choice between ``em`` and ``em_par`` is the caller's, as in
bulk.rs:155-159 (``threads > 4``): it only changes the stopping gate.
"""
from __future__ import annotations

import ctypes as C
import logging
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .types import AssignmentText, EMInfo, RunInfo, take_text_result


def _require_no_kde(em_info: EMInfo):
    if em_info.kde_model is not None:
        raise NotImplementedError(
            "kde_model is not supported: the KDE lives in the un-pinned `kders` crate and is only "
            "reachable through the hidden --use-kde flag (SURVEY.md section 8a note 4)")


def _dev(em_info: EMInfo):
    return em_info.eq_map.device_store(len(em_info.txp_info), em_info.device)


logger = logging.getLogger("oarfish_amd.em")
TRACE = 5  # the level that stands for the reference's `trace!` (below logging.DEBUG = 10)
logging.addLevelName(TRACE, "TRACE")
_LOGGED_ITERS = 1 << 20  # em / em_par record at most this many iterations (8 MB), whatever max_iter is


def history_log_records(history) -> List[Tuple[int, str]]:
    """The reference's convergence log of one run, from its rel_diff history (``DeviceStore.run_history``).

    do_em and em_par log ``iteration N; rel diff R`` after the increment of ``niter`` (em.rs:218) whenever
    ``N % 10 == 0``: ``info!`` when ``N % 100 == 0``, ``trace!`` otherwise (em.rs:219-233, :405-419).  ``N`` is
    formatted with ``Locale::en`` (``1,000``) and ``R`` is the rel_diff of the pass that ended with ``niter == N``,
    ``history[N - 1]``.  Returns ``[(level, message)]`` with ``logging.INFO`` or ``TRACE``, one per ``N % 10 == 0``
    up to ``len(history)``, in iteration order.  The pass through which a converged run leaves (``break``,
    em.rs:212-214) comes before the log line and is never logged: a caller passes ``history[:niter]``.

    The float's text is Python's ``repr`` (shortest round-trip, exponent notation for small values); Rust's ``{}``
    prints the same digits without an exponent (``0.00001`` for ``1e-05``).  That difference is left as it is.
    """
    out = []
    for n in range(10, len(history) + 1, 10):
        level = logging.INFO if n % 100 == 0 else TRACE
        out.append((level, f"iteration {n:,}; rel diff {float(history[n - 1])!r}"))
    return out


def _em_logged(em_info: EMInfo, gate: int) -> np.ndarray:
    """One EM run with the per-iteration record on (em.rs:270 / :326: ``do_log = true``), its lines handed to
    ``logging`` at the reference's cadence; the store's option is put back to off afterwards."""
    dev = _dev(em_info)
    dev.set_option(_lib.OEM_OPT_RUN_HISTORY, max(1, min(int(em_info.max_iter), _LOGGED_ITERS)))
    try:
        counts, info = dev.em_run(em_info.init_abundances, em_info.max_iter, em_info.convergence_thresh, gate)
        hist = dev.run_history(0)
    finally:
        dev.set_option(_lib.OEM_OPT_RUN_HISTORY, 0)
    em_info.last_run_info = info
    em_info.last_run_history = hist
    for level, msg in history_log_records(hist[:info.niter]):
        logger.log(level, msg)
    return counts


def em(em_info: EMInfo, _nthreads: int = 1) -> np.ndarray:
    """em.rs:262-271: serial-path semantics (stop when rel_diff < thresh and niter > 50).  Logs the reference's
    ``iteration N; rel diff R`` lines (``history_log_records``) to the logger ``oarfish_amd.em``; the run's whole
    rel_diff history is left in ``em_info.last_run_history``."""
    _require_no_kde(em_info)
    return _em_logged(em_info, 50)


def em_par(em_info: EMInfo, nthreads: int = 8) -> np.ndarray:
    """em.rs:320-447: parallel-path semantics (stop when rel_diff < thresh and niter > 1).  Logs as ``em`` does."""
    _require_no_kde(em_info)
    return _em_logged(em_info, 1)


def bootstrap(em_info: EMInfo, num_boot: int, nthreads: int = 1, seed: int = 0,
              row_weights: Optional[np.ndarray] = None) -> List[np.ndarray]:
    """em.rs:292-314.  Returns ``num_boot`` count vectors (``Vec<Vec<f64>>``).

    The reference seeds each replicate from the OS (em.rs:274), so its stream
    is not reproducible; here ``seed`` keys a counter-based device RNG, and
    ``row_weights`` (num_boot x n_reads multiplicities) injects the resamples.

    Silent, as the reference's replicates are (em.rs:289, ``do_log = false``); a caller who wants the
    replicates' rel_diff histories sets ``OEM_OPT_RUN_HISTORY`` on ``eq_map.device_store(...)`` and reads
    ``run_history(b)`` after the call.
    """
    _require_no_kde(em_info)
    out, _infos = _dev(em_info).bootstrap(num_boot, seed, row_weights, em_info.init_abundances,
                                          em_info.max_iter, em_info.convergence_thresh)
    return [out[b] for b in range(num_boot)]


def em_cells(cell_row_off: Sequence[int], boundaries, ref_ids, as_probabilities,
             coverage_probabilities, n_txps: int, max_iter: int = 1000,
             convergence_thresh: float = 1e-3, device: int = 0):
    """The per-cell contract of single_cell.rs:139-160, batched on the device.

    Every cell is an independent ``em::em(&emi, 1)`` with ``init_abundances: None``.
    Returns (counts[n_cells, n_txps] f64, [RunInfo]); the caller keeps ``v > 0`` as
    (col u32, val f32) triplets (single_cell.rs:155-160).
    """
    cell_row_off = np.ascontiguousarray(cell_row_off, dtype=np.uint64)
    boundaries = np.ascontiguousarray(boundaries, dtype=np.uint64)
    ref_ids = np.ascontiguousarray(ref_ids, dtype=np.uint32)
    as_probabilities = np.ascontiguousarray(as_probabilities, dtype=np.float32)
    cov = None if coverage_probabilities is None else np.ascontiguousarray(
        coverage_probabilities, dtype=np.float64)
    n_cells = len(cell_row_off) - 1
    n_reads = len(boundaries) - 1
    nnz = len(ref_ids)
    out = np.zeros((n_cells, n_txps), dtype=np.float64)
    infos = (_lib.RunInfoC * max(n_cells, 1))()
    _lib.check(_lib.lib().oem_em_run_cells(
        cell_row_off.ctypes.data, n_cells, boundaries.ctypes.data,
        ref_ids.ctypes.data if nnz else None, as_probabilities.ctypes.data if nnz else None,
        None if cov is None else cov.ctypes.data, n_reads, nnz, n_txps, device, max_iter,
        convergence_thresh, out.ctypes.data, C.addressof(infos)))
    return out, [RunInfo(i.niter, i.n_passes, bool(i.converged), i.rel_diff)
                 for i in list(infos)[:n_cells]]


def em_cells_sparse(cell_row_off: Sequence[int], boundaries, ref_ids, as_probabilities,
                    coverage_probabilities, n_txps: int, max_iter: int = 1000,
                    convergence_thresh: float = 1e-3, device: int = 0):
    """``em_cells`` with the result in the form single_cell.rs:151-160 keeps it: per cell the
    transcripts with ``v > 0`` as (col u32, val f32), ascending column, picked out on the device.

    Returns (indptr u64[n_cells + 1], cols u32, vals f32, [RunInfo]): cell c's entries are
    ``cols[indptr[c]:indptr[c + 1]]`` (``writers.csr_triplets`` turns them into the triplets of
    ``.count.mtx``).  Memory is proportional to the non-zeros, not to n_cells x n_txps.
    """
    cell_row_off = np.ascontiguousarray(cell_row_off, dtype=np.uint64)
    boundaries = np.ascontiguousarray(boundaries, dtype=np.uint64)
    ref_ids = np.ascontiguousarray(ref_ids, dtype=np.uint32)
    as_probabilities = np.ascontiguousarray(as_probabilities, dtype=np.float32)
    cov = None if coverage_probabilities is None else np.ascontiguousarray(
        coverage_probabilities, dtype=np.float64)
    n_cells = len(cell_row_off) - 1
    n_reads = len(boundaries) - 1
    nnz = len(ref_ids)
    L = _lib.lib()
    res = C.c_void_p()
    _lib.check(L.oem_em_run_cells_sparse(
        cell_row_off.ctypes.data, n_cells, boundaries.ctypes.data,
        ref_ids.ctypes.data if nnz else None, as_probabilities.ctypes.data if nnz else None,
        None if cov is None else cov.ctypes.data, n_reads, nnz, n_txps, device, max_iter,
        convergence_thresh, C.byref(res)))
    return _take_cells_result(res, n_cells)


def _take_cells_result(res, n_cells, L=None):
    """(indptr, cols, vals, [RunInfo]) of an ``oem_cells_result`` handle, which is released."""
    L = L or _lib.lib()
    try:
        nc, ne = C.c_uint32(0), C.c_uint64(0)
        _lib.check(L.oem_cells_result_dims(res, C.byref(nc), C.byref(ne)))
        indptr = np.zeros(int(nc.value) + 1, dtype=np.uint64)
        cols = np.empty(int(ne.value), dtype=np.uint32)
        vals = np.empty(int(ne.value), dtype=np.float32)
        infos = (_lib.RunInfoC * max(n_cells, 1))()
        _lib.check(L.oem_cells_result_copy(res, indptr.ctypes.data, cols.ctypes.data, vals.ctypes.data,
                                           C.addressof(infos)))
    finally:
        L.oem_cells_result_destroy(res)
    return indptr, cols, vals, [RunInfo(i.niter, i.n_passes, bool(i.converged), i.rel_diff)
                                for i in list(infos)[:n_cells]]


def count_matrix_text(indptr, cols, vals, n_txps: int, row_base: int = 0, prefix: bytes = b"", device: int = 0,
                      offsets: bool = True) -> AssignmentText:
    """write_function.rs:53-54: the `.count.mtx` text of the cells x transcripts matrix, formatted on the device
    (oem_count_matrix_text).  ``indptr, cols, vals`` is the CSR that ``em_cells_sparse``, ``em_cells_coverage_sparse``
    and ``CellsStream.finish`` return.  ``text`` is ``prefix`` (the banner and the dimension line) followed by one line
    ``"{row_base + cell + 1} {col + 1} {val}\n"`` per entry, the value as Rust's ``{}`` prints an f32 -- byte for byte
    what ``writers.write_single_cell_output`` writes for ``writers.csr_triplets(indptr, cols, vals)``.  ``line_off``:
    the byte offsets of the lines into the body (after the prefix); ``kept``: one per line.  ``offsets=False`` leaves
    those two ``None`` (a writer needs the text alone)."""
    indptr = np.ascontiguousarray(indptr, dtype=np.uint64)
    cols = np.ascontiguousarray(cols, dtype=np.uint32)
    vals = np.ascontiguousarray(vals, dtype=np.float32)
    if len(indptr) < 1:
        raise ValueError("indptr needs n_cells + 1 offsets")
    n_cells = len(indptr) - 1
    if len(cols) != len(vals) or int(indptr[-1]) != len(cols):
        raise ValueError("cols and vals must hold indptr[-1] entries each")
    prefix = bytes(prefix)
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.oem_count_matrix_text(indptr.ctypes.data, n_cells, cols.ctypes.data if len(cols) else None,
                                       vals.ctypes.data if len(vals) else None, n_txps, row_base,
                                       prefix if prefix else None, len(prefix), device, C.byref(h)))
    return take_text_result(L, h, offsets)


def cells_gene_counts(indptr, cols, vals, gene_of, n_genes: Optional[int] = None, device: int = 0):
    """The cells x transcripts CSR collapsed to cells x genes on the device (oem_cells_gene_counts; the rule is
    csrc/oem_gene_counts.h's).  ``indptr, cols, vals`` is the CSR ``em_cells_sparse`` and ``CellsStream.finish`` return,
    ``gene_of`` one gene id per transcript (``len(gene_of)`` is n_txps), ``n_genes=None`` means ``max(gene_of) + 1``.
    Per cell and gene the entries are added in CSR order in f64 and rounded once to f32; a gene entry exists wherever
    the cell has an entry of that gene; a cell's genes ascend.

    Returns ``(indptr_g u64[n_cells + 1], genes u32, vals_g f32)`` -- what ``count_matrix_text`` takes with ``n_genes``
    columns."""
    indptr = np.ascontiguousarray(indptr, dtype=np.uint64)
    cols = np.ascontiguousarray(cols, dtype=np.uint32)
    vals = np.ascontiguousarray(vals, dtype=np.float32)
    gene_of = np.asarray(gene_of)
    if gene_of.ndim != 1:
        raise ValueError("gene_of must be one gene id per transcript")
    if len(gene_of) and (not np.issubdtype(gene_of.dtype, np.integer) or int(gene_of.min()) < 0 or int(gene_of.max()) > 0xffffffff):
        raise ValueError("gene_of must hold integers in [0, 2^32)")
    gene_of = np.ascontiguousarray(gene_of, dtype=np.uint32)
    if len(indptr) < 1:
        raise ValueError("indptr needs n_cells + 1 offsets")
    n_cells = len(indptr) - 1
    if len(cols) != len(vals) or int(indptr[-1]) != len(cols):
        raise ValueError("cols and vals must hold indptr[-1] entries each")
    if n_genes is None:
        n_genes = int(gene_of.max()) + 1 if len(gene_of) else 0
    if not 0 <= int(n_genes) <= 0xffffffff:
        raise ValueError("n_genes must be in [0, 2^32)")
    L = _lib.lib()
    res = C.c_void_p()
    _lib.check(L.oem_cells_gene_counts(indptr.ctypes.data, n_cells, cols.ctypes.data if len(cols) else None,
                                       vals.ctypes.data if len(vals) else None,
                                       gene_of.ctypes.data if len(gene_of) else None, len(gene_of), int(n_genes), device,
                                       C.byref(res)))
    return _take_cells_result(res, n_cells, L)[:3]


_COVERAGE_MODELS = {"logistic": 0, "binomial": 1}


def _aln_record_dtype():
    from .builder import ALN_RECORD
    return ALN_RECORD


def cells_coverage_probs(cell_row_off: Sequence[int], boundaries, ref_ids, aln_start, aln_end, txp_len,
                         bin_width: int = 100, model: str = "binomial", growth_rate: float = 2.0,
                         device: int = 0) -> np.ndarray:
    """The coverage column of a single-cell ``--model-coverage`` run, every cell in one call.

    single_cell.rs:132-137 gives each cell its own coverage model: the cell's retained alignments are binned
    on pristine ``TranscriptInfo``s, ``binomial_continuous_prob`` turns the bins into probabilities and
    ``normalize_read_probs`` normalises the cell's reads.  Cells are given as in ``em_cells`` (one
    concatenated CSR plus ``cell_row_off``), with each alignment's ``aln_start`` / ``aln_end`` and the
    annotation's ``txp_len``.  ``model`` is ``"binomial"`` (the single-cell driver's) or ``"logistic"``
    (``growth_rate`` used).  Returns the nnz f64 ``coverage_probabilities`` of ``em_cells`` /
    ``em_cells_sparse``, in the caller's alignment order; a zero-span alignment gives NaN, as in the
    reference, and the cells EM drops its read.
    """
    if model not in _COVERAGE_MODELS:
        raise ValueError(f"model must be one of {sorted(_COVERAGE_MODELS)}, not {model!r}")
    cell_row_off = np.ascontiguousarray(cell_row_off, dtype=np.uint64)
    boundaries = np.ascontiguousarray(boundaries, dtype=np.uint64)
    ref_ids = np.ascontiguousarray(ref_ids, dtype=np.uint32)
    aln_start = np.ascontiguousarray(aln_start, dtype=np.uint32)
    aln_end = np.ascontiguousarray(aln_end, dtype=np.uint32)
    txp_len = np.ascontiguousarray(txp_len, dtype=np.uint64)
    nnz = len(ref_ids)
    if len(aln_start) != nnz or len(aln_end) != nnz:
        raise ValueError("ref_ids, aln_start and aln_end must have one entry per alignment")
    out = np.empty(nnz, dtype=np.float64)
    _lib.check(_lib.lib().oem_coverage_probs_cells_device(
        cell_row_off.ctypes.data, len(cell_row_off) - 1, boundaries.ctypes.data,
        ref_ids.ctypes.data if nnz else None, aln_start.ctypes.data if nnz else None,
        aln_end.ctypes.data if nnz else None, txp_len.ctypes.data, len(boundaries) - 1, nnz, len(txp_len),
        bin_width, _COVERAGE_MODELS[model], growth_rate, device, out.ctypes.data if nnz else None))
    return out


def em_cells_coverage_sparse(cell_row_off: Sequence[int], boundaries, ref_ids, as_probabilities, aln_start, aln_end,
                             txp_len, bin_width: int = 100, model: str = "binomial", growth_rate: float = 2.0,
                             max_iter: int = 1000, convergence_thresh: float = 1e-3, device: int = 0,
                             return_coverage: bool = False):
    """A single-cell ``--model-coverage`` run from the built store on, in one device call
    (single_cell.rs:117-160): every cell's own coverage model, then its EM, the entries ``v > 0`` kept.

    The result equals ``cells_coverage_probs`` on the same arguments followed by ``em_cells_sparse`` on that
    column, ``n_txps = len(txp_len)``; the column and the EM's weights stay on the device.  Returns
    ``(indptr, cols, vals, [RunInfo])`` as ``em_cells_sparse`` does, and with ``return_coverage`` also the
    nnz f64 coverage column the EM used (NaN for a zero-span alignment, whose read the EM drops).
    """
    if model not in _COVERAGE_MODELS:
        raise ValueError(f"model must be one of {sorted(_COVERAGE_MODELS)}, not {model!r}")
    cell_row_off = np.ascontiguousarray(cell_row_off, dtype=np.uint64)
    boundaries = np.ascontiguousarray(boundaries, dtype=np.uint64)
    ref_ids = np.ascontiguousarray(ref_ids, dtype=np.uint32)
    as_probabilities = np.ascontiguousarray(as_probabilities, dtype=np.float32)
    aln_start = np.ascontiguousarray(aln_start, dtype=np.uint32)
    aln_end = np.ascontiguousarray(aln_end, dtype=np.uint32)
    txp_len = np.ascontiguousarray(txp_len, dtype=np.uint64)
    nnz = len(ref_ids)
    if len(aln_start) != nnz or len(aln_end) != nnz or len(as_probabilities) != nnz:
        raise ValueError("ref_ids, as_probabilities, aln_start and aln_end must have one entry per alignment")
    n_cells = len(cell_row_off) - 1
    cov = np.empty(nnz, dtype=np.float64) if return_coverage else None
    res = C.c_void_p()
    _lib.check(_lib.lib().oem_em_run_cells_coverage_sparse(
        cell_row_off.ctypes.data, n_cells, boundaries.ctypes.data,
        ref_ids.ctypes.data if nnz else None, as_probabilities.ctypes.data if nnz else None,
        aln_start.ctypes.data if nnz else None, aln_end.ctypes.data if nnz else None, txp_len.ctypes.data,
        len(boundaries) - 1, nnz, len(txp_len), bin_width, _COVERAGE_MODELS[model], growth_rate, device, max_iter,
        convergence_thresh, cov.ctypes.data if cov is not None and nnz else None, C.byref(res)))
    out = _take_cells_result(res, n_cells)
    return (*out, cov) if return_coverage else out


def _discard_tables(L, res, n_cells):
    """The per-cell discard tables of a result that came from records, as a list of dicts."""
    from .builder import discard_dict
    dts = (_lib.DiscardTableC * max(n_cells, 1))()
    rc = L.oem_cells_result_discard_tables(res, C.addressof(dts))
    if rc != _lib.OEM_OK:
        msg = L.oem_last_error()
        raise _lib.OemError(rc, msg.decode("utf-8", "replace") if msg else "")
    return [discard_dict(dts[c]) for c in range(n_cells)]


_COLLATE_MODES = {"sort": _lib.OEM_COLLATE_SORT, "adjacent": _lib.OEM_COLLATE_ADJACENT}


def collate_names(names, cell_rec_off, secondary=None, mode: str = "sort", device: int = 0):
    """The records of cells collated by read name on the device (``oem_collate_names``; alignment_parser.rs:170-241,
    and :301-437 with ``mode="adjacent"``).

    ``names``: the records' read names, whatever ``types.pack_read_names`` accepts (a sequence of ``str`` / ``bytes`` or
    a ``(blob, offsets)`` pair); none is empty or holds a 0 byte.  ``cell_rec_off``: cell ``c`` owns the records
    ``cell_rec_off[c] : cell_rec_off[c + 1]``.  ``secondary``: one flag per record (the SAM secondary flag), or None.

    Returns ``(order, group_off, cell_group_off)``: per cell, ``order`` holds the cell's record indices sorted by
    (name bytes, secondary, index) -- the identity under ``"adjacent"`` --; ``records[order]`` with ``group_off`` and
    ``cell_group_off`` is what ``em_cells_records_sparse`` and ``CellsStream.push_records`` take.
    """
    from .types import pack_read_names
    if mode not in _COLLATE_MODES:
        raise ValueError(f"mode must be one of {sorted(_COLLATE_MODES)}, not {mode!r}")
    cell_rec_off = np.ascontiguousarray(cell_rec_off, dtype=np.uint64)
    if cell_rec_off.ndim != 1 or len(cell_rec_off) < 1:
        raise ValueError("cell_rec_off needs n_cells + 1 entries")
    n = len(names[1]) - 1 if isinstance(names, tuple) and len(names) == 2 and not isinstance(names[1], (str, bytes)) else len(names)
    blob, off = pack_read_names(names, n)
    sec = None
    if secondary is not None:
        sec = np.ascontiguousarray(np.asarray(secondary) != 0, dtype=np.uint8)
        if len(sec) != n:
            raise ValueError("secondary must have one entry per record")
    order = np.empty(max(n, 1), dtype=np.uint32)
    group_off = np.empty(n + 1, dtype=np.uint64)
    cell_group_off = np.empty(len(cell_rec_off), dtype=np.uint64)
    n_groups = C.c_uint64(0)
    if n and not len(blob):
        blob = np.zeros(1, dtype=np.uint8)   # (every name is empty: the call says so)
    _lib.check(_lib.lib().oem_collate_names(
        blob.ctypes.data if n else None, off.ctypes.data,
        None if sec is None or not n else sec.ctypes.data, n, cell_rec_off.ctypes.data, len(cell_rec_off) - 1,
        _COLLATE_MODES[mode], device, order.ctypes.data, group_off.ctypes.data, C.byref(n_groups), cell_group_off.ctypes.data))
    return order[:n], group_off[:int(n_groups.value) + 1].copy(), cell_group_off


def _n_packed(names) -> int:
    """How many names ``pack_read_names`` will find in ``names``."""
    return len(names[1]) - 1 if isinstance(names, tuple) and len(names) == 2 and not isinstance(names[1], (str, bytes)) else len(names)


def collate_barcodes(barcodes, device: int = 0):
    """The cells of records that are in any order (``oem_collate_barcodes``; the reference wants a barcode's records
    adjacent: single_cell.rs:196-213, alignment_parser.rs:244-299).

    ``barcodes``: one barcode per record, whatever ``types.pack_read_names`` accepts; none is empty or holds a 0 byte.
    Returns ``(order, cell_rec_off)``: ``order`` puts the records cell by cell -- cells in the order of their first
    record, records in input order inside a cell --, cell ``c`` owns ``order[cell_rec_off[c] : cell_rec_off[c + 1]]``.
    ``records[order]`` and ``names`` in that order, with ``cell_rec_off``, are what ``collate_names`` and
    ``em_cells_records_sparse(..., names=)`` take.
    """
    from .types import pack_read_names
    n = _n_packed(barcodes)
    blob, off = pack_read_names(barcodes, n)
    order = np.empty(max(n, 1), dtype=np.uint32)
    cell_rec_off = np.empty(n + 1, dtype=np.uint64)
    n_cells = C.c_uint64(0)
    if n and not len(blob):
        blob = np.zeros(1, dtype=np.uint8)   # (every barcode is empty: the call says so)
    _lib.check(_lib.lib().oem_collate_barcodes(blob.ctypes.data if n else None, off.ctypes.data, n, device, order.ctypes.data,
                                               cell_rec_off.ctypes.data, C.byref(n_cells)))
    return order[:n], cell_rec_off[:int(n_cells.value) + 1].copy()


class BarcodeRuleC(C.Structure):
    """``oem_barcode_rule``."""
    _fields_ = [("labels", C.c_void_p), ("label_off", C.c_void_p), ("n_labels", C.c_uint32), ("multi", C.c_uint32),
                ("alphabet", C.c_void_p), ("n_alphabet", C.c_uint32), ("reserved", C.c_uint32)]


def _barcode_rule(whitelist, multi, alphabet):
    """(the ``oem_barcode_rule`` of a call, the arrays it points into: the whitelist's blob and offsets, the alphabet)."""
    from .types import pack_read_names
    w = _n_packed(whitelist)
    if w < 1:
        raise ValueError("whitelist needs one label at least")
    blob, off = pack_read_names(whitelist, w)
    alpha = None
    if alphabet is not None:
        if isinstance(alphabet, str):
            alphabet = alphabet.encode()
        alpha = np.frombuffer(bytes(alphabet), dtype=np.uint8).copy()
        if not 1 <= len(alpha) <= 8:
            raise ValueError("alphabet needs 1 to 8 bytes")
    if not len(blob):
        blob = np.zeros(1, dtype=np.uint8)   # (every label is empty: the call says so)
    rule = BarcodeRuleC(blob.ctypes.data, off.ctypes.data, w, int(bool(multi)), None if alpha is None else alpha.ctypes.data,
                        0 if alpha is None else len(alpha), 0)
    return rule, (blob, off, alpha)


def correct_barcodes(barcodes, whitelist, multi: bool = False, alphabet=b"ACGT", device: int = 0):
    """Raw cell barcodes matched against a whitelist, with one-mismatch correction (``oem_correct_barcodes``; the
    reference wants every record to carry a corrected barcode, docs/index.md:308-312).

    ``barcodes``: one raw barcode (``CR``) per record, whatever ``types.pack_read_names`` accepts; the empty string where
    the tag is missing.  ``whitelist``: the chemistry's permit list, distinct labels of 1 to 64 bytes, likewise.  A
    barcode that is a label is exact; one that differs from labels of its length in exactly one position, the label's byte
    there being in ``alphabet``, is corrected to that label if it is the only one -- with ``multi`` (STARsolo's
    ``1MM_multi`` without qualities) also to the one that has strictly the most exact records among several.  Everything
    else is rejected: no neighbour, ambiguous, missing.

    Returns ``(wl_id, status, order, cell_rec_off, counts)``: every record's label index (``0xffffffff``: rejected) and
    ``OEM_BARCODE_*`` status, the cells of the accepted records as ``collate_barcodes`` gives them (``order`` holds the
    accepted records only), and the records of each of the five statuses."""
    from .types import pack_read_names
    n = _n_packed(barcodes)
    blob, off = pack_read_names(barcodes, n)
    rule, _keep = _barcode_rule(whitelist, multi, alphabet)
    wl_id = np.empty(max(n, 1), dtype=np.uint32)
    status = np.empty(max(n, 1), dtype=np.uint8)
    order = np.empty(max(n, 1), dtype=np.uint32)
    cell_rec_off = np.empty(n + 1, dtype=np.uint64)
    counts = np.zeros(5, dtype=np.uint64)
    n_cells, n_acc = C.c_uint64(0), C.c_uint64(0)
    if n and not len(blob):
        blob = np.zeros(1, dtype=np.uint8)   # (every barcode is missing)
    _lib.check(_lib.lib().oem_correct_barcodes(C.addressof(rule), blob.ctypes.data if n else None, off.ctypes.data, n, device,
                                               wl_id.ctypes.data, status.ctypes.data, order.ctypes.data, cell_rec_off.ctypes.data,
                                               C.byref(n_cells), C.byref(n_acc), counts.ctypes.data))
    return wl_id[:n], status[:n], order[:int(n_acc.value)].copy(), cell_rec_off[:int(n_cells.value) + 1].copy(), counts


def dedup_umis(umis, order, group_off, cell_group_off, flags=None, device: int = 0):
    """The PCR duplicates among the reads of a collated order (``oem_dedup_umis``; the reference wants its single-cell
    input deduplicated already, docs/index.md:308-312).

    ``umis``: one UMI per INPUT record, whatever ``types.pack_read_names`` accepts; a record without a ``UB`` tag has the
    empty string, none holds a 0 byte.  ``order`` / ``group_off`` / ``cell_group_off``: a collated order as
    ``collate_barcodes`` and ``collate_names`` leave it (``order[k]`` is the input index at position ``k``, a group is a
    read).  ``flags``: the records' flag words (``records["flags"]``), or None when no record is unmapped.

    A read takes part when the UMI of its first record is not empty and that record is mapped; inside a cell the reads
    that take part and have byte-identical UMIs are one molecule, whose first read survives.  Returns ``(dup, survivor,
    cell_dups)``: ``dup[g]`` 0 / 1, ``survivor[g]`` the surviving group of a duplicate and ``g`` otherwise, ``cell_dups[c]``
    the duplicates of cell ``c``.  ``drop_groups`` applies ``dup``.
    """
    from .types import pack_read_names
    n = _n_packed(umis)
    blob, off = pack_read_names(umis, n)
    order = np.ascontiguousarray(order, dtype=np.uint32)
    group_off = np.ascontiguousarray(group_off, dtype=np.uint64)
    cell_group_off = np.ascontiguousarray(cell_group_off, dtype=np.uint64)
    if group_off.ndim != 1 or len(group_off) < 1:
        raise ValueError("group_off needs n_groups + 1 entries")
    if cell_group_off.ndim != 1 or len(cell_group_off) < 1:
        raise ValueError("cell_group_off needs n_cells + 1 entries")
    fl = None
    if flags is not None:
        fl = np.ascontiguousarray(flags, dtype=np.uint32)
        if len(fl) != n:
            raise ValueError("flags must have one entry per record")
    n_groups, n_cells = len(group_off) - 1, len(cell_group_off) - 1
    dup = np.zeros(max(n_groups, 1), dtype=np.uint8)
    survivor = np.zeros(max(n_groups, 1), dtype=np.uint64)
    cell_dups = np.zeros(max(n_cells, 1), dtype=np.uint64)
    if not len(blob):
        blob = np.zeros(1, dtype=np.uint8)
    _lib.check(_lib.lib().oem_dedup_umis(
        blob.ctypes.data, off.ctypes.data, None if fl is None or not n else fl.ctypes.data, n, order.ctypes.data if len(order) else None,
        len(order), group_off.ctypes.data, n_groups, cell_group_off.ctypes.data, n_cells, device, dup.ctypes.data, survivor.ctypes.data,
        cell_dups.ctypes.data))
    return dup[:n_groups], survivor[:n_groups], cell_dups[:n_cells]


class UmiRuleC(C.Structure):
    """``oem_umi_rule``."""
    _fields_ = [("gene_of", C.c_void_p), ("n_txps", C.c_uint32), ("correct", C.c_uint32)]


def _umi_rule(gene_of, correct):
    """(the ``oem_umi_rule`` of a call, the array it points into)."""
    gene = None if gene_of is None else np.ascontiguousarray(gene_of, dtype=np.uint32)
    if gene is not None and gene.ndim != 1:
        raise ValueError("gene_of needs one gene id per transcript")
    return UmiRuleC(None if gene is None or not len(gene) else gene.ctypes.data, 0 if gene is None else len(gene), int(bool(correct))), gene


def dedup_umis_rule(umis, order, group_off, cell_group_off, flags=None, ref_id=None, gene_of=None, correct: bool = False,
                    device: int = 0):
    """``dedup_umis`` under a UMI rule (``oem_dedup_umis_rule``): gene-aware keys and one-mismatch correction.

    ``gene_of``: None, or one gene id per transcript; ``ref_id`` (the records' ``records["ref_id"]``) is then required,
    and the key of a molecule is (cell, gene of the read's first record, UMI): the same UMI in two genes of one cell is
    two molecules.  ``correct``: a UMI one mismatch away from a more abundant UMI of the same cell and gene is an error of
    it (Cell Ranger's rule; the most abundant such neighbour, among equals the smallest bytes; chains are followed to
    their root).  With both at their defaults this is ``dedup_umis``.  Returns ``(dup, survivor, cell_dups,
    cell_corrected)``: ``cell_corrected[c]`` counts the reads of cell ``c`` whose UMI was corrected.
    """
    from .types import pack_read_names
    n = _n_packed(umis)
    blob, off = pack_read_names(umis, n)
    order = np.ascontiguousarray(order, dtype=np.uint32)
    group_off = np.ascontiguousarray(group_off, dtype=np.uint64)
    cell_group_off = np.ascontiguousarray(cell_group_off, dtype=np.uint64)
    if group_off.ndim != 1 or len(group_off) < 1:
        raise ValueError("group_off needs n_groups + 1 entries")
    if cell_group_off.ndim != 1 or len(cell_group_off) < 1:
        raise ValueError("cell_group_off needs n_cells + 1 entries")
    fl = rid = None
    if flags is not None:
        fl = np.ascontiguousarray(flags, dtype=np.uint32)
        if len(fl) != n:
            raise ValueError("flags must have one entry per record")
    if ref_id is not None:
        rid = np.ascontiguousarray(ref_id, dtype=np.uint32)
        if len(rid) != n:
            raise ValueError("ref_id must have one entry per record")
    if gene_of is not None and rid is None:
        raise ValueError("gene_of needs ref_id: a read's gene is its first record's transcript's")
    rule, _gene = _umi_rule(gene_of, correct)
    n_groups, n_cells = len(group_off) - 1, len(cell_group_off) - 1
    dup = np.zeros(max(n_groups, 1), dtype=np.uint8)
    survivor = np.zeros(max(n_groups, 1), dtype=np.uint64)
    cell_dups = np.zeros(max(n_cells, 1), dtype=np.uint64)
    cell_corrected = np.zeros(max(n_cells, 1), dtype=np.uint64)
    if not len(blob):
        blob = np.zeros(1, dtype=np.uint8)
    _lib.check(_lib.lib().oem_dedup_umis_rule(
        C.addressof(rule), blob.ctypes.data, off.ctypes.data, None if fl is None or not n else fl.ctypes.data,
        None if rid is None or not n else rid.ctypes.data, n, order.ctypes.data if len(order) else None, len(order), group_off.ctypes.data,
        n_groups, cell_group_off.ctypes.data, n_cells, device, dup.ctypes.data, survivor.ctypes.data, cell_dups.ctypes.data,
        cell_corrected.ctypes.data))
    return dup[:n_groups], survivor[:n_groups], cell_dups[:n_cells], cell_corrected[:n_cells]


def drop_groups(order, group_off, cell_group_off, dup):
    """A collated order without the groups marked in ``dup``: the NumPy compaction behind ``dedup_umis``.  Returns
    ``(order, group_off, cell_group_off, cell_rec_off)`` of the deduplicated collation -- the marked groups' positions are
    removed, everything else stays in place."""
    order = np.asarray(order)
    group_off = np.ascontiguousarray(group_off, dtype=np.uint64)
    cell_group_off = np.ascontiguousarray(cell_group_off, dtype=np.uint64)
    keep = np.asarray(dup) == 0
    if len(keep) != len(group_off) - 1:
        raise ValueError("dup must have one entry per group")
    sizes = np.diff(group_off.astype(np.int64))
    new_group_off = np.zeros(int(keep.sum()) + 1, dtype=np.uint64)
    np.cumsum(sizes[keep], out=new_group_off[1:])
    kept_before = np.zeros(len(keep) + 1, dtype=np.uint64)
    np.cumsum(keep, out=kept_before[1:])
    new_cell_group_off = kept_before[cell_group_off.astype(np.int64)]
    return (np.ascontiguousarray(order[np.repeat(keep, sizes)]), new_group_off, new_cell_group_off,
            new_group_off[new_cell_group_off.astype(np.int64)])


def gather_names(names, idx):
    """``names`` (a ``(blob, offsets)`` pair) in the order ``idx``: the NumPy gather of a variable-length blob."""
    blob, off = np.asarray(names[0]), np.ascontiguousarray(names[1], dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    lens = (off[1:] - off[:-1])[idx]
    new_off = np.zeros(len(idx) + 1, dtype=np.uint64)
    np.cumsum(lens, out=new_off[1:])
    src = np.repeat(off[:-1][idx] - new_off[:-1].astype(np.int64), lens) + np.arange(int(new_off[-1]), dtype=np.int64)
    return np.ascontiguousarray(blob[src]), new_off


def _em_cells_records_whitelist(F, txp_len, records, coverage, max_iter, conv_thresh, device, names, sec, barcodes, umis, collate, mode,
                                gene_of, umi_correct, whitelist, barcode_multi):
    """``em_cells_records_sparse(..., barcodes=, names=, whitelist=)`` behind its packing: the one call
    (``collate="device"``, oem_em_run_cells_records_whitelist_sparse), or the five steps it replaces.  Both return the
    ten values of the UMI-rule form and ``wl_id``, ``status``, ``counts``."""
    from .types import pack_read_names
    n = len(records)
    if collate == "host":
        wl_id, status, _, _, counts = correct_barcodes(barcodes, whitelist, multi=barcode_multi, device=device)
        keep = np.flatnonzero(wl_id != _lib.OEM_BARCODE_NO_ID)
        labels = pack_read_names(whitelist, _n_packed(whitelist))
        um = (np.zeros(0, dtype=np.uint8), np.zeros(len(keep) + 1, dtype=np.uint64)) if umis is None else gather_names(umis, keep)
        out = _em_cells_records_umis(F, txp_len, records[keep], coverage, max_iter, conv_thresh, device, gather_names(names, keep),
                                     None if sec is None else np.ascontiguousarray(sec[keep]), gather_names(labels, wl_id[keep]), um,
                                     "device", mode, gene_of, umi_correct, always_rule=True)
        return (*out[:6], keep.astype(np.uint32)[out[6]], *out[7:], wl_id, status, counts)
    blob, off = names
    bc_blob, bc_off = barcodes
    one = np.zeros(1, dtype=np.uint8)
    blob, bc_blob = (b if len(b) else one for b in (blob, bc_blob))
    um_blob, um_off = (None, None) if umis is None else (umis[0] if len(umis[0]) else one, umis[1])
    rule, _keep = _barcode_rule(whitelist, barcode_multi, None)
    umi_rule, _gene = _umi_rule(gene_of, umi_correct)
    model, bin_width, growth_rate = _coverage_args(coverage)
    order = np.empty(max(n, 1), dtype=np.uint32)
    kept = np.zeros(max(n, 1), dtype=np.uint32)
    cell_rec_off = np.empty(n + 1, dtype=np.uint64)
    cell_dups = np.zeros(max(n, 1), dtype=np.uint64)
    cell_corrected = np.zeros(max(n, 1), dtype=np.uint64)
    wl_id = np.empty(max(n, 1), dtype=np.uint32)
    status = np.empty(max(n, 1), dtype=np.uint8)
    counts = np.zeros(5, dtype=np.uint64)
    n_groups, n_cells, n_surv = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    L = _lib.lib()
    res = C.c_void_p()
    _lib.check(L.oem_em_run_cells_records_whitelist_sparse(
        C.addressof(rule), C.addressof(umi_rule), C.addressof(F), txp_len.ctypes.data, len(txp_len), records.ctypes.data if n else None, n,
        bc_blob.ctypes.data if n else None, bc_off.ctypes.data, blob.ctypes.data if n else None, off.ctypes.data,
        None if sec is None or not n else sec.ctypes.data, None if um_blob is None else um_blob.ctypes.data,
        None if um_off is None else um_off.ctypes.data, _COLLATE_MODES[mode], bin_width, model, growth_rate, device, max_iter, conv_thresh,
        order.ctypes.data, C.byref(n_surv), cell_rec_off.ctypes.data, C.byref(n_cells), None, C.byref(n_groups), None, kept.ctypes.data,
        cell_dups.ctypes.data, cell_corrected.ctypes.data, wl_id.ctypes.data, status.ctypes.data, counts.ctypes.data, C.byref(res)))
    nc = int(n_cells.value)
    try:
        tables = _discard_tables(L, res, nc)
    except BaseException:
        L.oem_cells_result_destroy(res)
        raise
    return (*_take_cells_result(res, nc, L), kept[:int(n_groups.value)].copy(), tables, order[:int(n_surv.value)].copy(),
            cell_rec_off[:nc + 1].copy(), cell_dups[:nc].copy(), cell_corrected[:nc].copy(), wl_id[:n], status[:n], counts)


def _em_cells_records_umis(F, txp_len, records, coverage, max_iter, conv_thresh, device, names, sec, barcodes, umis, collate, mode,
                           gene_of=None, umi_correct=False, always_rule=False):
    """``em_cells_records_sparse(..., barcodes=, names=, umis=)`` behind its packing: the one call
    (``collate="device"``, oem_em_run_cells_records_umis_sparse), or the seven steps it replaces.  With ``gene_of`` or
    ``umi_correct`` the one call is oem_em_run_cells_records_umis_rule_sparse, the join's fifth step ``dedup_umis_rule``,
    and ``cell_corrected`` is a tenth value."""
    with_rule = gene_of is not None or bool(umi_correct) or always_rule
    blob, off = names
    bc_blob, bc_off = barcodes
    um_blob, um_off = umis
    n = len(records)
    if collate == "host":
        order_bc, cell_rec_off = collate_barcodes((bc_blob, bc_off), device=device)
        order_names, group_off, cell_group_off = collate_names(gather_names((blob, off), order_bc), cell_rec_off,
                                                               None if sec is None else sec[order_bc], mode=mode, device=device)
        order = order_bc[order_names]
        cell_corrected = None
        if with_rule:
            dup, _, cell_dups, cell_corrected = dedup_umis_rule((um_blob, um_off), order, group_off, cell_group_off, flags=records["flags"],
                                                                ref_id=records["ref_id"], gene_of=gene_of, correct=umi_correct,
                                                                device=device)
        else:
            dup, _, cell_dups = dedup_umis((um_blob, um_off), order, group_off, cell_group_off, flags=records["flags"], device=device)
        order, group_off, cell_group_off, cell_rec_off = drop_groups(order, group_off, cell_group_off, dup)
        out = _em_cells_records_plain(F, txp_len, records[order], group_off, cell_group_off, coverage, max_iter, conv_thresh, device)
        return (*out, order, cell_rec_off, cell_dups) + ((cell_corrected,) if with_rule else ())
    one = np.zeros(1, dtype=np.uint8)
    blob, bc_blob, um_blob = (b if len(b) else one for b in (blob, bc_blob, um_blob))
    model, bin_width, growth_rate = _coverage_args(coverage)
    order = np.empty(max(n, 1), dtype=np.uint32)
    kept = np.zeros(max(n, 1), dtype=np.uint32)
    cell_rec_off = np.empty(n + 1, dtype=np.uint64)
    cell_dups = np.zeros(max(n, 1), dtype=np.uint64)
    n_groups, n_cells, n_surv = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    L = _lib.lib()
    res = C.c_void_p()
    head = (C.addressof(F), txp_len.ctypes.data, len(txp_len), records.ctypes.data if n else None, n,
            bc_blob.ctypes.data if n else None, bc_off.ctypes.data, blob.ctypes.data if n else None, off.ctypes.data,
            None if sec is None or not n else sec.ctypes.data, um_blob.ctypes.data, um_off.ctypes.data, _COLLATE_MODES[mode], bin_width, model,
            growth_rate, device, max_iter, conv_thresh, order.ctypes.data, C.byref(n_surv), cell_rec_off.ctypes.data, C.byref(n_cells), None,
            C.byref(n_groups), None, kept.ctypes.data, cell_dups.ctypes.data)
    if with_rule:
        rule, _gene = _umi_rule(gene_of, umi_correct)
        cell_corrected = np.zeros(max(n, 1), dtype=np.uint64)
        _lib.check(L.oem_em_run_cells_records_umis_rule_sparse(C.addressof(rule), *head, cell_corrected.ctypes.data, C.byref(res)))
    else:
        _lib.check(L.oem_em_run_cells_records_umis_sparse(*head, C.byref(res)))
    nc = int(n_cells.value)
    try:
        tables = _discard_tables(L, res, nc)
    except BaseException:
        L.oem_cells_result_destroy(res)
        raise
    return (*_take_cells_result(res, nc, L), kept[:int(n_groups.value)].copy(), tables, order[:int(n_surv.value)].copy(),
            cell_rec_off[:nc + 1].copy(), cell_dups[:nc].copy()) + ((cell_corrected[:nc].copy(),) if with_rule else ())


def _em_cells_records_barcodes(F, txp_len, records, coverage, max_iter, conv_thresh, device, names, secondary, barcodes, collate, mode,
                               umis=None, gene_of=None, umi_correct=False, whitelist=None, barcode_multi=False):
    """``em_cells_records_sparse(..., names=, barcodes=)``: the one call (``collate="device"``), or the join it replaces."""
    from .types import pack_read_names
    records = np.ascontiguousarray(records, dtype=_aln_record_dtype())
    n = len(records)
    if _n_packed(names) != n:
        raise ValueError("names must have one entry per record")
    if _n_packed(barcodes) != n:
        raise ValueError("barcodes must have one entry per record")
    blob, off = pack_read_names(names, n)
    bc_blob, bc_off = pack_read_names(barcodes, n)
    sec = None
    if secondary is not None:
        sec = np.ascontiguousarray(np.asarray(secondary) != 0, dtype=np.uint8)
        if len(sec) != n:
            raise ValueError("secondary must have one entry per record")
    if umis is not None and _n_packed(umis) != n:
        raise ValueError("umis must have one entry per record")
    if whitelist is not None:
        return _em_cells_records_whitelist(F, txp_len, records, coverage, max_iter, conv_thresh, device, (blob, off), sec, (bc_blob, bc_off),
                                           None if umis is None else pack_read_names(umis, n), collate, mode, gene_of, umi_correct,
                                           whitelist, barcode_multi)
    if umis is not None:
        return _em_cells_records_umis(F, txp_len, records, coverage, max_iter, conv_thresh, device, (blob, off), sec, (bc_blob, bc_off),
                                      pack_read_names(umis, n), collate, mode, gene_of, umi_correct)
    if collate == "host":   # the four steps the one call replaces
        order_bc, cell_rec_off = collate_barcodes((bc_blob, bc_off), device=device)
        out = _em_cells_records_names(F, txp_len, records[order_bc], cell_rec_off, coverage, max_iter, conv_thresh, device,
                                      gather_names((blob, off), order_bc), None if sec is None else sec[order_bc], mode)
        return (*out[:6], order_bc[out[6]], cell_rec_off)
    if n and not len(blob):
        blob = np.zeros(1, dtype=np.uint8)
    if n and not len(bc_blob):
        bc_blob = np.zeros(1, dtype=np.uint8)
    model, bin_width, growth_rate = _coverage_args(coverage)
    order = np.empty(max(n, 1), dtype=np.uint32)
    kept = np.zeros(max(n, 1), dtype=np.uint32)
    cell_rec_off = np.empty(n + 1, dtype=np.uint64)
    n_groups, n_cells = C.c_uint64(0), C.c_uint64(0)
    L = _lib.lib()
    res = C.c_void_p()
    _lib.check(L.oem_em_run_cells_records_barcodes_sparse(
        C.addressof(F), txp_len.ctypes.data, len(txp_len), records.ctypes.data if n else None, n,
        bc_blob.ctypes.data if n else None, bc_off.ctypes.data, blob.ctypes.data if n else None, off.ctypes.data,
        None if sec is None or not n else sec.ctypes.data, _COLLATE_MODES[mode], bin_width, model, growth_rate, device, max_iter,
        conv_thresh, order.ctypes.data, cell_rec_off.ctypes.data, C.byref(n_cells), None, C.byref(n_groups), None,
        kept.ctypes.data, C.byref(res)))
    nc = int(n_cells.value)
    try:
        tables = _discard_tables(L, res, nc)
    except BaseException:
        L.oem_cells_result_destroy(res)
        raise
    return (*_take_cells_result(res, nc, L), kept[:int(n_groups.value)].copy(), tables, order[:n], cell_rec_off[:nc + 1].copy())


def _coverage_args(coverage):
    """(model, bin_width, growth_rate) of a ``coverage`` dict as the records calls take it; None = no model."""
    if coverage is None:
        return -1, 0, 0.0
    name = coverage.get("model", "binomial")
    if name not in _COVERAGE_MODELS:
        raise ValueError(f"model must be one of {sorted(_COVERAGE_MODELS)}, not {name!r}")
    return _COVERAGE_MODELS[name], coverage.get("bin_width", 100), coverage.get("growth_rate", 2.0)


def _em_cells_records_names(F, txp_len, records, cell_rec_off, coverage, max_iter, conv_thresh, device, names, secondary, mode):
    """``em_cells_records_sparse(..., names=, collate="device")``: the one call."""
    from .types import pack_read_names
    records = np.ascontiguousarray(records, dtype=_aln_record_dtype())
    n = len(records)
    cell_rec_off = np.ascontiguousarray(cell_rec_off, dtype=np.uint64)
    if cell_rec_off.ndim != 1 or len(cell_rec_off) < 1:
        raise ValueError("cell_rec_off needs n_cells + 1 entries")
    n_names = len(names[1]) - 1 if isinstance(names, tuple) and len(names) == 2 and not isinstance(names[1], (str, bytes)) else len(names)
    if n_names != n:
        raise ValueError("names must have one entry per record")
    blob, off = pack_read_names(names, n)
    sec = None
    if secondary is not None:
        sec = np.ascontiguousarray(np.asarray(secondary) != 0, dtype=np.uint8)
        if len(sec) != n:
            raise ValueError("secondary must have one entry per record")
    if n and not len(blob):
        blob = np.zeros(1, dtype=np.uint8)   # (every name is empty: the call says so)
    n_cells = len(cell_rec_off) - 1
    model, bin_width, growth_rate = _coverage_args(coverage)
    order = np.empty(max(n, 1), dtype=np.uint32)
    kept = np.zeros(max(n, 1), dtype=np.uint32)
    n_groups = C.c_uint64(0)
    L = _lib.lib()
    res = C.c_void_p()
    _lib.check(L.oem_em_run_cells_records_names_sparse(
        C.addressof(F), txp_len.ctypes.data, len(txp_len), records.ctypes.data if n else None, n,
        blob.ctypes.data if n else None, off.ctypes.data, None if sec is None or not n else sec.ctypes.data,
        cell_rec_off.ctypes.data, n_cells, _COLLATE_MODES[mode], bin_width, model, growth_rate, device, max_iter, conv_thresh,
        order.ctypes.data, None, C.byref(n_groups), None, kept.ctypes.data, C.byref(res)))
    try:
        tables = _discard_tables(L, res, n_cells)
    except BaseException:
        L.oem_cells_result_destroy(res)
        raise
    return (*_take_cells_result(res, n_cells, L), kept[:int(n_groups.value)].copy(), tables, order[:n])


def em_cells_records_sparse(filters, txp_len, records, group_off, cell_group_off, coverage=None, max_iter: int = 1000,
                            conv_thresh: float = 1e-3, device: int = 0, names=None, secondary=None, collate: str = "host",
                            mode: str = "sort", barcodes=None, umis=None, gene_of=None, umi_correct: bool = False, whitelist=None,
                            barcode_multi: bool = False):
    """A single-cell run from the cells' alignment records on, in one device call (single_cell.rs:104-188,
    oem_em_run_cells_records_sparse): AlignmentFilters::filter into every cell's own store, the per-cell coverage
    model if asked, em::em, the entries ``v > 0`` kept.  The filtered CSR never exists on the host.

    ``records`` / ``group_off`` are a batch as ``StoreBuilder.add_groups`` takes it (one group per read); cell ``c``
    owns the groups ``cell_group_off[c] : cell_group_off[c + 1]``.  ``coverage``: None, or
    ``dict(bin_width=..., model="binomial" | "logistic", growth_rate=...)``.  Returns ``(indptr, cols, vals,
    [RunInfo], kept, discard_tables)``: the first four as ``em_cells_sparse`` returns them, ``kept`` what
    ``add_groups`` returns per group, ``discard_tables`` one dict per cell -- that cell's builder's discard table.

    ``names`` (with ``secondary``, as ``collate_names`` takes them): the records are collated by barcode only.
    ``group_off`` is then ignored and ``cell_group_off`` is read as ``cell_rec_off``; the call collates the records on
    the device, runs on ``records[order]`` and appends ``order`` to what it returns (``kept`` counts the groups of the
    collated order).  ``collate="host"`` joins the two device calls here: ``collate_names``, ``records[order]`` with
    NumPy, then the records call.  ``collate="device"`` is one call (oem_em_run_cells_records_names_sparse): names and
    records go up in input order and the order is applied on the device; same seven values.  ``mode`` is
    ``collate_names``': ``"adjacent"`` for input that is name-collated already.

    ``barcodes`` (one per record, as ``collate_barcodes`` takes them; ``names`` is then required and ``group_off`` /
    ``cell_group_off`` must be None): the records are in any order at all and the cells are found from the barcodes.
    ``collate="device"`` is one call (oem_em_run_cells_records_barcodes_sparse): barcodes, names and records go up in
    input order, nothing is gathered on the host.  ``collate="host"`` joins ``collate_barcodes``, the NumPy gathers of
    records, names and ``secondary``, and the names call: the path the one call replaces.  Both return the seven
    values of the names form -- ``order`` is the composed one, the input index of every collated position -- and
    ``cell_rec_off`` as an eighth.

    ``umis`` (one per record, as ``dedup_umis`` takes them; goes with ``barcodes``): the input is not UMI-deduplicated
    (the reference wants it to be, docs/index.md:308-312).  Inside every cell the reads whose first records carry the
    same UMI are one molecule and only the first of them is counted; the records' own ``flags`` say which are unmapped.
    ``collate="device"`` is one call (oem_em_run_cells_records_umis_sparse): the duplicates leave the collation on the
    device and their records are never gathered.  ``collate="host"`` is the join it replaces: ``collate_barcodes``, the
    NumPy gathers, ``collate_names``, the composed order, ``dedup_umis``, ``drop_groups``, the records call.  Both
    return the eight values of the barcodes form over the DEDUPLICATED collation -- ``order`` holds the surviving
    positions only -- and ``cell_dups``, the duplicates dropped from every cell, as a ninth.

    ``gene_of`` (one gene id per transcript) and ``umi_correct`` (both go with ``umis``) are the UMI rule of
    ``dedup_umis_rule``: molecules keyed by (cell, gene of the read's first record, UMI), and UMIs one mismatch away from
    a more abundant UMI of the same cell and gene counted as errors of it.  With either, ``collate="device"`` is
    oem_em_run_cells_records_umis_rule_sparse, ``collate="host"`` the same join with ``dedup_umis_rule``, and
    ``cell_corrected``, the reads of every cell whose UMI was corrected, is a tenth value.  With both at their defaults
    nothing changes.

    ``whitelist`` (goes with ``barcodes``; ``barcode_multi`` goes with it): the barcodes are RAW (``CR`` tags) and are
    matched against the whitelist with one-mismatch correction first, as ``correct_barcodes`` does it; the records that
    are rejected belong to no cell, and their names, UMIs and ``ref_id`` are never looked at.  ``collate="device"`` is one
    call (oem_em_run_cells_records_whitelist_sparse); ``collate="host"`` the join it replaces: ``correct_barcodes``, the
    rejected records dropped with NumPy, the labels' bytes as barcodes, the UMI-rule one call, ``order`` mapped back.
    Both return the ten values of the UMI-rule form (with or without ``umis``; ``order`` holds input indices of accepted
    records only) and then ``wl_id``, ``status`` and ``counts`` as ``correct_barcodes`` returns them.  ``whitelist=None``
    changes nothing.
    """
    from .builder import filters_c
    if collate not in ("host", "device"):
        raise ValueError(f"collate must be 'host' or 'device', not {collate!r}")
    if mode not in _COLLATE_MODES:
        raise ValueError(f"mode must be one of {sorted(_COLLATE_MODES)}, not {mode!r}")
    if names is None and secondary is not None:
        raise ValueError("secondary goes with names")
    if umis is not None and barcodes is None:
        raise ValueError("umis goes with barcodes: the molecules of a cell are found where the cells are")
    if umis is None and (gene_of is not None or umi_correct):
        raise ValueError("gene_of and umi_correct go with umis: they are the rule the UMIs are deduplicated by")
    if whitelist is not None and barcodes is None:
        raise ValueError("whitelist goes with barcodes: it is what the raw barcodes are corrected against")
    if whitelist is None and barcode_multi:
        raise ValueError("barcode_multi goes with whitelist")
    if barcodes is not None:
        if cell_group_off is not None or group_off is not None:
            raise ValueError("with barcodes the cells are found by the call: group_off and cell_group_off must be None")
        if names is None:
            raise ValueError("barcodes needs names")
    F = filters_c(filters)
    txp_len = np.ascontiguousarray(txp_len, dtype=np.uint64)
    if barcodes is not None:
        return _em_cells_records_barcodes(F, txp_len, records, coverage, max_iter, conv_thresh, device, names, secondary, barcodes,
                                          collate, mode, umis, gene_of, umi_correct, whitelist, barcode_multi)
    if names is not None and collate == "device":
        return _em_cells_records_names(F, txp_len, records, cell_group_off, coverage, max_iter, conv_thresh, device, names,
                                       secondary, mode)
    order = None
    if names is not None:
        order, group_off, cell_group_off = collate_names(names, cell_group_off, secondary, mode=mode, device=device)
        records = np.ascontiguousarray(records, dtype=_aln_record_dtype())
        if len(records) != len(order):
            raise ValueError("names must have one entry per record")
        records = records[order]
    out = _em_cells_records_plain(F, txp_len, records, group_off, cell_group_off, coverage, max_iter, conv_thresh, device)
    return out if order is None else (*out, order)


def _em_cells_records_plain(F, txp_len, records, group_off, cell_group_off, coverage, max_iter, conv_thresh, device):
    """``em_cells_records_sparse`` on collated records: oem_em_run_cells_records_sparse and its six values."""
    from .builder import check_batch
    records, group_off = check_batch(records, group_off)
    cell_group_off = np.ascontiguousarray(cell_group_off, dtype=np.uint64)
    if cell_group_off.ndim != 1 or len(cell_group_off) < 1:
        raise ValueError("cell_group_off needs n_cells + 1 entries")
    n_groups, n_cells = len(group_off) - 1, len(cell_group_off) - 1
    model, bin_width, growth_rate = _coverage_args(coverage)
    kept = np.zeros(n_groups, dtype=np.uint32)
    L = _lib.lib()
    res = C.c_void_p()
    _lib.check(L.oem_em_run_cells_records_sparse(
        C.addressof(F), txp_len.ctypes.data, len(txp_len), records.ctypes.data if len(records) else None,
        group_off.ctypes.data, n_groups, cell_group_off.ctypes.data, n_cells, bin_width, model, growth_rate, device,
        max_iter, conv_thresh, kept.ctypes.data, C.byref(res)))
    try:
        tables = _discard_tables(L, res, n_cells)
    except BaseException:
        L.oem_cells_result_destroy(res)
        raise
    return (*_take_cells_result(res, n_cells, L), kept, tables)


class CellsStream:
    """A per-cell session (``oem_cells_stream_*``): cells are pushed one by one, from any number of threads, as
    they become available -- the way single_cell.rs:96-193 produces them -- and the library runs them in batched
    groups on the device while later cells still arrive.

    ``coverage``: None, or ``dict(bin_width=..., model="binomial" | "logistic", growth_rate=..., txp_len=...)`` for
    the per-cell coverage model of ``em_cells_coverage_sparse`` (cells are then pushed with their coordinates).
    ``group_nnz`` / ``group_cells`` / ``max_staged_nnz``: 0 = the library's defaults.  Use as a context manager;
    leaving the block before ``finish()`` cancels the session.

    ``push`` returns the cell's ticket: cell ``k`` of the result is the cell with ticket ``k``.  ``finish()`` returns
    what ``em_cells_sparse`` returns.  ``push`` is thread-safe and releases the GIL while the library works.

    ``filters`` with ``txp_len`` makes it a RECORDS session (``oem_cells_stream_set_filters``): cells are pushed as
    their alignment records with ``push_records`` and filtered on the device, as ``em_cells_records_sparse`` does; the
    budgets then count records, and ``discard_tables()`` gives every cell's discard table after ``finish()``.

    ``barcodes=True`` (with ``filters``) makes it a BARCODED session (``oem_cells_stream_set_barcodes``): the input is a
    barcode-collated stream of records, pushed with ``push_batch`` in batches cut at any record position.  The device
    skips the unmapped records, cuts a cell where the barcode changes, carries the open cell from batch to batch and
    runs the closed cells in groups while later batches arrive.  ``mode`` is ``collate_names``' (applied inside every
    cell).  ``finish()`` returns the usual four values -- what ``em_cells_records_sparse(names=, collate="device")`` gives
    for the surviving records with the cells the barcodes cut -- and ``cells()`` what the session found.

    ``collated=False`` (with ``barcodes=True``) is the ANY-ORDER barcoded session
    (``oem_cells_stream_set_barcodes_any_order``): the batches' records come in any order, a barcode that comes back is
    the same cell, and cells are numbered by their first surviving record.  Every batch's barcodes are interned on the
    device against a table of the labels seen so far; nothing runs before ``finish()``, which gives exactly what
    ``em_cells_records_sparse(..., barcodes=, collate="device")`` gives on the surviving records.  ``info()`` then has
    ``arena_bytes``, ``barcode_misses`` and ``barcode_table_slots`` (0 on every other session).

    ``umis=True`` (with ``barcodes=True``, either form) is a UMI session (``oem_cells_stream_set_umis``): ``push_batch``
    takes one UMI per record, every group of cells is deduplicated on the device behind its name collation
    (``dedup_umis``' rule), ``cells()`` describes the deduplicated collation and gains ``cell_dups``, and ``info()`` has
    ``umi_dup_reads`` and ``umi_dup_records`` (0 on every other session).  The any-order form gives exactly what
    ``em_cells_records_sparse(..., barcodes=, names=, umis=)`` gives on the surviving records.

    ``gene_of`` (one gene id per transcript) and ``umi_correct`` (both go with ``umis=True``) are the UMI rule of
    ``dedup_umis_rule`` in every group of the session (``oem_cells_stream_set_umi_rule``): molecules keyed by (cell, gene
    of the read's first record, UMI), and UMIs one mismatch away from a more abundant one corrected to it.  With
    ``umi_correct``, ``cells()`` gains ``cell_corrected`` and ``info()["umi_corrected_reads"]`` counts them.  The any-order
    form gives exactly what ``em_cells_records_sparse(..., umis=, gene_of=, umi_correct=)`` gives on the surviving records.

    ``whitelist`` (with ``barcodes=True, collated=False``; ``barcode_multi`` and ``barcode_alphabet`` go with it) is the
    WHITELIST session (``oem_cells_stream_set_whitelist``): the batches' barcodes are RAW (``CR`` tags) and every batch is
    matched against the whitelist on the device, as ``correct_barcodes`` does it.  A record rejected in its batch is
    dropped there -- its name, UMI and ``ref_id`` are never looked at --, and under ``barcode_multi`` a barcode between
    several labels waits for ``finish()``, which decides it with the complete counts.  Unmapped records take no part.
    ``finish()`` gives exactly what ``em_cells_records_sparse(..., barcodes=, whitelist=)`` gives on the mapped records;
    ``cells()`` describes the accepted records, its ``barcodes`` are the whitelist's labels, and it gains ``cell_wl_id``,
    ``cell_bc_corrected`` and ``counts``; ``info()`` has ``barcode_rejected`` and ``barcode_deferred``.  One difference
    from the one call: a deferred record is checked in its batch, so an error in its name, UMI or ``ref_id`` is the
    session's even if ``finish()`` then rejects the record.
    """

    def __init__(self, n_txps: int, max_iter: int = 1000, conv_thresh: float = 1e-3, coverage=None, device: int = 0,
                 group_nnz: int = 0, group_cells: int = 0, max_staged_nnz: int = 0, filters=None, txp_len=None,
                 barcodes: bool = False, mode: str = "sort", collated: bool = True, umis: bool = False, gene_of=None,
                 umi_correct: bool = False, whitelist=None, barcode_multi: bool = False, barcode_alphabet=None):
        if whitelist is not None and not barcodes:
            raise ValueError("whitelist goes with barcodes=True: it is what a barcoded session's raw barcodes are corrected against")
        if whitelist is not None and collated:
            raise ValueError("whitelist goes with collated=False: corrected barcodes would scatter one label over many cells of a "
                             "collated session")
        if whitelist is None and (barcode_multi or barcode_alphabet is not None):
            raise ValueError("barcode_multi goes with whitelist (and so does barcode_alphabet)")
        if umis and not barcodes:
            raise ValueError("umis=True goes with barcodes=True: only a barcoded session takes UMIs")
        if (gene_of is not None or umi_correct) and not umis:
            raise ValueError("gene_of and umi_correct go with umis=True: they are the rule the UMIs are deduplicated by")
        if gene_of is not None and (np.ndim(gene_of) != 1 or len(gene_of) != n_txps):
            raise ValueError("gene_of must have n_txps entries: one gene id per transcript")
        if not collated and not barcodes:
            raise ValueError("collated=False goes with barcodes=True: only a barcoded session finds its cells itself")
        if barcodes and filters is None:
            raise ValueError("a barcoded session is a records session: it needs filters and txp_len")
        if mode not in _COLLATE_MODES:
            raise ValueError(f"mode must be one of {sorted(_COLLATE_MODES)}, not {mode!r}")
        if filters is not None and txp_len is None and coverage is not None:
            txp_len = coverage.get("txp_len")
        if filters is not None and txp_len is None:
            raise ValueError("a records session needs txp_len with its filters")
        if filters is not None and coverage is not None and "txp_len" not in coverage:
            coverage = dict(coverage, txp_len=txp_len)
        self._tables = None
        self._cells = None
        self._barcoded = bool(barcodes)
        self._any_order = bool(barcodes) and not collated
        self._umis = bool(umis)
        self._umi_correct = bool(umi_correct)
        self._whitelist = whitelist is not None
        self._device = device
        records_txp_len = txp_len
        o = _lib.CellsStreamOptsC()
        o.n_txps, o.device, o.max_iter, o.conv_thresh = n_txps, device, max_iter, conv_thresh
        o.group_nnz, o.group_cells, o.max_staged_nnz = group_nnz, group_cells, max_staged_nnz
        txp_len = None
        if coverage is not None:
            model = coverage.get("model", "binomial")
            if model not in _COVERAGE_MODELS:
                raise ValueError(f"model must be one of {sorted(_COVERAGE_MODELS)}, not {model!r}")
            txp_len = np.ascontiguousarray(coverage["txp_len"], dtype=np.uint64)
            if len(txp_len) != n_txps:
                raise ValueError("coverage['txp_len'] must have n_txps entries")
            o.coverage, o.bin_width, o.model = 1, coverage.get("bin_width", 100), _COVERAGE_MODELS[model]
            o.growth_rate = coverage.get("growth_rate", 2.0)
        self._coverage = coverage is not None
        self._L = _lib.lib()   # (a handle belongs to the library that made it)
        self._h = C.c_void_p()
        _lib.check(self._L.oem_cells_stream_create(C.byref(o), None if txp_len is None else txp_len.ctypes.data,
                                                   C.byref(self._h)))
        if filters is not None:
            from .builder import filters_c
            F = filters_c(filters)
            tl = np.ascontiguousarray(records_txp_len, dtype=np.uint64)
            if len(tl) != n_txps:
                self.close()
                raise ValueError("txp_len must have n_txps entries")
            try:
                self.set_filters(F, tl)
                if barcodes:
                    set_barcodes = self._L.oem_cells_stream_set_barcodes if collated else self._L.oem_cells_stream_set_barcodes_any_order
                    self._check(set_barcodes(self._h, _COLLATE_MODES[mode]))
                    if umis:
                        self._check(self._L.oem_cells_stream_set_umis(self._h))
                    if gene_of is not None or umi_correct:
                        rule, _gene = _umi_rule(gene_of, umi_correct)   # (the session copies gene_of)
                        self._check(self._L.oem_cells_stream_set_umi_rule(self._h, C.addressof(rule)))
                    if whitelist is not None:
                        wl_rule, _wl = _barcode_rule(whitelist, barcode_multi, barcode_alphabet)   # (the session copies the arrays)
                        self._check(self._L.oem_cells_stream_set_whitelist(self._h, C.addressof(wl_rule)))
            except BaseException:
                self.close()
                raise

    def set_filters(self, filters, txp_len) -> None:
        """Turns a fresh session into a records session (``oem_cells_stream_set_filters``)."""
        from .builder import filters_c
        if not self._h:
            raise _lib.OemError(_lib.OEM_ERR_STATE, "CellsStream is closed")
        F = filters_c(filters)
        tl = np.ascontiguousarray(txp_len, dtype=np.uint64)
        self._check(self._L.oem_cells_stream_set_filters(self._h, C.addressof(F), tl.ctypes.data))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self) -> None:
        if self._h:
            self._L.oem_cells_stream_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:   # pragma: no cover - interpreter shutdown
            pass

    def _check(self, rc: int) -> None:
        if rc != _lib.OEM_OK:
            msg = self._L.oem_last_error()
            raise _lib.OemError(rc, msg.decode("utf-8", "replace") if msg else "")

    def push(self, row_ptr, tid, as_prob, start=None, end=None) -> int:
        if not self._h:
            raise _lib.OemError(_lib.OEM_ERR_STATE, "CellsStream is closed")
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
        tid = np.ascontiguousarray(tid, dtype=np.uint32)
        as_prob = np.ascontiguousarray(as_prob, dtype=np.float32)
        nnz = len(tid)
        if len(as_prob) != nnz:
            raise ValueError("tid and as_prob must have one entry per alignment")
        if len(row_ptr) < 1:
            raise ValueError("row_ptr needs n_reads + 1 entries")
        if start is not None:
            start = np.ascontiguousarray(start, dtype=np.uint32)
            end = np.ascontiguousarray(end, dtype=np.uint32)
            if len(start) != nnz or len(end) != nnz:
                raise ValueError("start and end must have one entry per alignment")
        ticket = C.c_uint64(0)
        self._check(self._L.oem_cells_stream_push(
            self._h, row_ptr.ctypes.data, tid.ctypes.data if nnz else None, as_prob.ctypes.data if nnz else None,
            None if start is None or not nnz else start.ctypes.data, None if start is None or not nnz else end.ctypes.data,
            len(row_ptr) - 1, nnz, C.byref(ticket)))
        return int(ticket.value)

    def push_records(self, records, group_off=None, names=None, secondary=None):
        """One cell of a records session: its reads' records as a batch (``StoreBuilder.add_groups``' arguments).
        Returns the cell's ticket.

        With ``names`` (and ``secondary``, as ``collate_names`` takes them) the cell's records are in any order and
        ``group_off`` is not given: the cell is collated on the device first, ``records[order]`` is pushed, and the call
        returns ``(ticket, order)``."""
        if not self._h:
            raise _lib.OemError(_lib.OEM_ERR_STATE, "CellsStream is closed")
        records = np.ascontiguousarray(records, dtype=_aln_record_dtype())
        if names is not None:
            order, group_off, _ = collate_names(names, [0, len(records)], secondary, device=self._device)
            return self.push_records(records[order], group_off), order
        if secondary is not None:
            raise ValueError("secondary goes with names")
        if group_off is None:
            raise ValueError("push_records needs group_off, or the records' names")
        group_off = np.ascontiguousarray(group_off, dtype=np.uint64)
        if group_off.ndim != 1 or len(group_off) < 1:
            raise ValueError("group_off needs n_groups + 1 entries")
        if int(group_off.max()) > len(records):
            raise ValueError("group_off runs past the end of records")
        ticket = C.c_uint64(0)
        self._check(self._L.oem_cells_stream_push_records(self._h, records.ctypes.data if len(records) else None,
                                                          group_off.ctypes.data, len(group_off) - 1, C.byref(ticket)))
        return int(ticket.value)

    def push_batch(self, records, barcodes, names, secondary=None, umis=None) -> int:
        """One batch of a barcoded session: ``records`` with one barcode and one read name each -- ``(blob, offsets)``
        pairs or sequences of ``bytes``, as ``collate_barcodes`` and ``collate_names`` take them -- and their
        ``secondary`` flags.  The batch may start and end anywhere: inside a cell, inside a read.  Returns the batch's
        ticket; the session's input is its batches in ticket order.  Thread-safe; releases the GIL.

        A UMI session takes ``umis`` likewise, one per record (``b""``: no UMI); ``None`` means every UMI of the batch
        is empty.  Giving ``umis`` to a session without them is a ``ValueError``."""
        from .types import pack_read_names
        if not self._h:
            raise _lib.OemError(_lib.OEM_ERR_STATE, "CellsStream is closed")
        records = np.ascontiguousarray(records, dtype=_aln_record_dtype())
        n = len(records)
        if _n_packed(barcodes) != n:
            raise ValueError("barcodes must have one entry per record")
        if _n_packed(names) != n:
            raise ValueError("names must have one entry per record")
        bc_blob, bc_off = pack_read_names(barcodes, n)
        blob, off = pack_read_names(names, n)
        sec = None
        if secondary is not None:
            sec = np.ascontiguousarray(np.asarray(secondary) != 0, dtype=np.uint8)
            if len(sec) != n:
                raise ValueError("secondary must have one entry per record")
        ticket = C.c_uint64(0)
        with_umis = getattr(self, "_umis", False)
        if umis is not None and not with_umis:
            raise ValueError("umis go to a UMI session: CellsStream(..., barcodes=True, umis=True)")
        if with_umis:
            if umis is None:
                u_blob, u_off = np.zeros(0, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64)
            else:
                if _n_packed(umis) != n:
                    raise ValueError("umis must have one entry per record")
                u_blob, u_off = pack_read_names(umis, n)
            self._check(self._L.oem_cells_stream_push_barcodes_umis(
                self._h, records.ctypes.data if n else None, n, bc_blob.ctypes.data if len(bc_blob) else None, bc_off.ctypes.data,
                blob.ctypes.data if len(blob) else None, off.ctypes.data, None if sec is None or not n else sec.ctypes.data,
                u_blob.ctypes.data if len(u_blob) else None, u_off.ctypes.data, C.byref(ticket)))
            return int(ticket.value)
        self._check(self._L.oem_cells_stream_push_barcodes(
            self._h, records.ctypes.data if n else None, n, bc_blob.ctypes.data if len(bc_blob) else None, bc_off.ctypes.data,
            blob.ctypes.data if len(blob) else None, off.ctypes.data, None if sec is None or not n else sec.ctypes.data,
            C.byref(ticket)))
        return int(ticket.value)

    def cells(self) -> dict:
        """After ``finish()`` of a barcoded session: ``barcodes`` (the cells' labels, a list of ``bytes``, in cell order),
        ``cell_rec_off`` (positions among the surviving records), ``order`` (uint64: the index in the pushed stream of the
        record at every collated position), ``group_off``, ``cell_group_off``, ``kept`` and ``n_unmapped``.  A UMI
        session: all of them describe the deduplicated collation, and ``cell_dups`` (uint64) are the duplicate reads that
        every cell lost; with ``umi_correct`` also ``cell_corrected`` (uint64), the reads of every cell whose UMI was
        corrected.  A whitelist session: they describe the accepted records, ``barcodes`` are the whitelist's labels, and
        ``cell_wl_id`` (uint32: every cell's label index), ``cell_bc_corrected`` (uint64: the records of every cell whose
        barcode was corrected) and ``counts`` (uint64, the mapped records of each ``OEM_BARCODE_*`` status) come with them."""
        if self._cells is None:
            raise _lib.OemError(_lib.OEM_ERR_STATE, "cells(): a finished barcoded session has them")
        return self._cells

    def _take_cells(self) -> dict:
        d = [C.c_uint64(0) for _ in range(5)]
        self._check(self._L.oem_cells_stream_barcodes_dims(self._h, *[C.byref(x) for x in d]))
        nc, m, ng, nb, n_unmapped = (int(x.value) for x in d)
        blob = np.zeros(max(nb, 1), dtype=np.uint8)
        bc_off = np.zeros(nc + 1, dtype=np.uint64)
        cell_rec_off = np.zeros(nc + 1, dtype=np.uint64)
        order = np.zeros(max(m, 1), dtype=np.uint64)
        group_off = np.zeros(ng + 1, dtype=np.uint64)
        cell_group_off = np.zeros(nc + 1, dtype=np.uint64)
        kept = np.zeros(max(ng, 1), dtype=np.uint32)
        self._check(self._L.oem_cells_stream_barcodes_copy(
            self._h, blob.ctypes.data, bc_off.ctypes.data, cell_rec_off.ctypes.data, order.ctypes.data, group_off.ctypes.data,
            cell_group_off.ctypes.data, kept.ctypes.data))
        raw = blob.tobytes()
        out = dict(barcodes=[raw[int(bc_off[c]):int(bc_off[c + 1])] for c in range(nc)], cell_rec_off=cell_rec_off,
                   order=order[:m], group_off=group_off, cell_group_off=cell_group_off, kept=kept[:ng], n_unmapped=n_unmapped)
        if self._umis:
            dups = np.zeros(max(nc, 1), dtype=np.uint64)
            self._check(self._L.oem_cells_stream_umis_copy(self._h, dups.ctypes.data))
            out["cell_dups"] = dups[:nc]
        if self._umi_correct:
            corrected = np.zeros(max(nc, 1), dtype=np.uint64)
            self._check(self._L.oem_cells_stream_umi_rule_copy(self._h, corrected.ctypes.data))
            out["cell_corrected"] = corrected[:nc]
        if self._whitelist:
            wl_id = np.zeros(max(nc, 1), dtype=np.uint32)
            bc_corrected = np.zeros(max(nc, 1), dtype=np.uint64)
            counts = np.zeros(5, dtype=np.uint64)
            self._check(self._L.oem_cells_stream_whitelist_copy(self._h, wl_id.ctypes.data, bc_corrected.ctypes.data, counts.ctypes.data))
            out["cell_wl_id"], out["cell_bc_corrected"], out["counts"] = wl_id[:nc], bc_corrected[:nc], counts
        return out

    def finish(self):
        """(indptr, cols, vals, [RunInfo]) of every pushed cell, in ticket order (a barcoded session: of every cell it
        found, in input order)."""
        if not self._h:
            raise _lib.OemError(_lib.OEM_ERR_STATE, "CellsStream is closed")
        res = C.c_void_p()
        self._check(self._L.oem_cells_stream_finish(self._h, C.byref(res)))
        if self._barcoded:
            try:
                self._cells = self._take_cells()
            except BaseException:
                self._L.oem_cells_result_destroy(res)
                raise
        nc = C.c_uint32(0)
        self._check(self._L.oem_cells_result_dims(res, C.byref(nc), None))
        dts = (_lib.DiscardTableC * max(int(nc.value), 1))()
        if self._L.oem_cells_result_discard_tables(res, C.addressof(dts)) == _lib.OEM_OK:   # (a records session)
            from .builder import discard_dict
            self._tables = [discard_dict(dts[c]) for c in range(int(nc.value))]
        return _take_cells_result(res, int(nc.value), self._L)

    def discard_tables(self):
        """After ``finish()`` of a records session: one dict per cell, in ticket order -- the discard table of that
        cell's own builder."""
        if self._tables is None:
            raise _lib.OemError(_lib.OEM_ERR_STATE, "discard_tables(): a finished records session has them")
        return self._tables

    def info(self) -> dict:
        keys = dict(cells=_lib.OEM_CELLS_STREAM_INFO_CELLS, alignments=_lib.OEM_CELLS_STREAM_INFO_ALIGNMENTS,
                    groups=_lib.OEM_CELLS_STREAM_INFO_GROUPS,
                    groups_before_finish=_lib.OEM_CELLS_STREAM_INFO_GROUPS_BEFORE_FINISH,
                    blocked_s=_lib.OEM_CELLS_STREAM_INFO_BLOCKED_US, groups_batched=_lib.OEM_CELLS_STREAM_INFO_GROUPS_BATCHED,
                    arena_bytes=_lib.OEM_CELLS_STREAM_INFO_ARENA_BYTES, barcode_misses=_lib.OEM_CELLS_STREAM_INFO_BARCODE_MISSES,
                    barcode_table_slots=_lib.OEM_CELLS_STREAM_INFO_BARCODE_TABLE_SLOTS,
                    umi_dup_reads=_lib.OEM_CELLS_STREAM_INFO_UMI_DUP_READS, umi_dup_records=_lib.OEM_CELLS_STREAM_INFO_UMI_DUP_RECORDS,
                    umi_corrected_reads=_lib.OEM_CELLS_STREAM_INFO_UMI_CORRECTED_READS,
                    barcode_rejected=_lib.OEM_CELLS_STREAM_INFO_BARCODE_REJECTED,
                    barcode_deferred=_lib.OEM_CELLS_STREAM_INFO_BARCODE_DEFERRED)
        out = {}
        for name, key in keys.items():
            v = C.c_uint64(0)
            self._check(self._L.oem_cells_stream_info(self._h, key, C.byref(v)))
            out[name] = v.value * 1e-6 if name == "blocked_s" else int(v.value)
        return out


def cells_last_timing():
    """(device milliseconds of the batched EM loops, batched passes launched) of this thread's last
    ``em_cells`` call -- oem_cells_last_timing; bench.py's per-cell roofline."""
    ms, n = C.c_float(0), C.c_uint64(0)
    _lib.check(_lib.lib().oem_cells_last_timing(C.byref(ms), C.byref(n)))
    return float(ms.value), int(n.value)
