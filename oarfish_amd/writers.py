"""Result files in the reference's on-disk formats.

Host-side formatting only; every number written here comes out of the device engine
(`em` / `em_par` / `bootstrap` / `DeviceStore.aux_counts` / `DeviceStore.assignment_probs`).

  write_output               write_function.rs:72-148   <out>.meta_info.json, .quant, .ambig_info.tsv
  write_output_device        the same three files, the lines of `.quant` and `.ambig_info.tsv` formatted on the device
                             (quant_text, ambig_text)
  write_infrep_file          write_function.rs:199-209, parquet_utils.rs:15-44, bulk.rs:181-193
  write_out_prob             write_function.rs:226-340  <out>.prob
  write_out_prob_device      the same file, its body formatted on the device (DeviceStore.assignment_text); with
                             compressed=True <out>.prob.lz4 (:243-263, 334-337), formatted AND compressed on the
                             device (DeviceStore.assignment_text_lz4): one valid LZ4 frame of the same bytes, which
                             departs from the reference's file in its encoding only -- independent 64 KiB blocks,
                             per-block checksums instead of a content checksum, a fast greedy parse instead of HC
                             level 4 -- so it is larger than the reference's and every LZ4 frame decoder reads it
  write_single_cell_output   write_function.rs:25-69    <out>.count.mtx, .features.txt (+ .barcodes.txt,
                             single_cell.rs:176-178)
  write_single_cell_output_device  the same files, the matrix lines formatted on the device (em.count_matrix_text)

Numbers are printed the way Rust's `{}` prints them (shortest digits that round-trip, never an
exponent, no trailing ".0" -- `rust_display`), so a `.quant` written here is byte-identical to the
reference's for equal counts.
"""
from __future__ import annotations

import json
import math
import os
from typing import Iterable, Optional, Sequence

import numpy as np


def rust_display(x, f32: bool = False) -> str:
    """`format!("{}", x)` of an f64 (or f32): shortest round-trip digits, positional notation."""
    x = np.float32(x) if f32 else np.float64(x)
    if np.isnan(x):
        return "NaN"
    if np.isinf(x):
        return "inf" if x > 0 else "-inf"
    return np.format_float_positional(x, unique=True, trim="-")


def with_additional_extension(output: str, ext: str) -> str:
    """path_tools::WithAdditionalExtension: append, never replace."""
    return str(output) + ext


def _make_parent(output: str) -> None:  # write_function.rs:32-40
    parent = os.path.dirname(str(output))
    if parent:
        os.makedirs(parent, exist_ok=True)


_QUANT_HEADER = "tname\tlen\tnum_reads\n"
_AMBIG_HEADER = "unique_reads\tambig_reads\ttotal_reads\n"


def _write_meta_info(output: str, info: dict) -> None:
    """The parent directory and `.meta_info.json` (write_function.rs:78-102), what every form of `write_output` starts
    with."""
    _make_parent(output)
    with open(with_additional_extension(output, ".meta_info.json"), "w") as fh:
        json.dump(info, fh, indent=2)                       # serde_json to_writer_pretty


def write_output(output: str, info: dict, names: Sequence[str], lens: Sequence[int], counts,
                 unique_counts, total_counts) -> None:
    """write_function.rs:72-148: `.meta_info.json`, `.quant` (tname, len, num_reads) and
    `.ambig_info.tsv` (unique, ambig = total - unique saturating, total)."""
    if not (len(names) == len(lens) == len(counts) == len(unique_counts) == len(total_counts)):
        raise ValueError("write_output: per-transcript columns differ in length")
    _write_meta_info(output, info)
    with open(with_additional_extension(output, ".quant"), "w") as fh:
        fh.write(_QUANT_HEADER)
        for n, l, c in zip(names, lens, counts):
            fh.write(f"{n}\t{int(l)}\t{rust_display(c)}\n")
    with open(with_additional_extension(output, ".ambig_info.tsv"), "w") as fh:
        fh.write(_AMBIG_HEADER)
        for u, t in zip(unique_counts, total_counts):
            u, t = int(u), int(t)
            fh.write(f"{u}\t{max(t - u, 0)}\t{t}\n")


def pack_names(names):
    """Transcript names as the C ABI takes them: (blob uint8, offsets uint64[n + 1]).  ``names`` is a sequence of
    ``str`` / ``bytes`` or already such a pair.  A list of ``str`` is joined and encoded in one go (no work per name in
    the interpreter); anything else goes through ``types.pack_read_names``."""
    from .types import pack_read_names

    if not (isinstance(names, tuple) and len(names) == 2 and not isinstance(names[1], (str, bytes))):
        names = list(names)
        n = len(names)
        try:
            joined = np.frombuffer("\n".join(names).encode("utf-8"), dtype=np.uint8)
        except TypeError:                                   # bytes among them
            joined = None
        if joined is not None and n:
            is_nl = joined == 10
            ends = np.flatnonzero(is_nl)
            if len(ends) == n - 1:                          # (a name with a newline in it: the slow way, and the library refuses it)
                off = np.zeros(n + 1, dtype=np.uint64)
                off[1:n] = ends - np.arange(n - 1)
                off[n] = len(joined) - (n - 1)
                return np.ascontiguousarray(joined[~is_nl]), off
        return pack_read_names(names, n)
    return pack_read_names(names, len(names[1]) - 1)


def quant_text_lines(names, lens, counts, prefix: bytes = b"", device: int = 0, offsets: bool = True):
    """write_function.rs:104-120 on the device (oem_quant_text): ``text`` is ``prefix`` followed by one line
    ``name\tlen\tcount\n`` per transcript, the count as Rust's ``{}`` prints an f64 -- byte for byte what
    ``write_output`` writes into `.quant` after its header line.  ``names``: a sequence of ``str`` / ``bytes`` or a pair
    ``(blob, offsets)``.  ``line_off``: the byte offsets of the lines into the body (after the prefix); ``kept``: one
    per line; ``offsets=False`` leaves those two ``None``.  A count that is not finite, or a name with a tab or a
    newline in it, is an ``OemError`` (OEM_ERR_ARG)."""
    import ctypes as C

    from . import _lib
    from .types import take_text_result

    blob, off = pack_names(names)
    n = len(off) - 1
    lens = np.ascontiguousarray(lens, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.float64)
    if len(lens) != n or len(counts) != n:
        raise ValueError("quant_text: names, lens and counts differ in length")
    if len(blob) == 0:
        blob = np.zeros(1, dtype=np.uint8)                  # a non-NULL pointer: the names exist, they are all empty
    prefix = bytes(prefix)
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.oem_quant_text(blob.ctypes.data, off.ctypes.data, lens.ctypes.data if n else None,
                                counts.ctypes.data if n else None, n, prefix if prefix else None, len(prefix), device,
                                C.byref(h)))
    return take_text_result(L, h, offsets)


def ambig_text_lines(unique, total, prefix: bytes = b"", device: int = 0, offsets: bool = True):
    """write_function.rs:122-145 on the device (oem_ambig_text): ``prefix`` and one line
    ``unique\tambig\ttotal\n`` per transcript, ``ambig = total - unique`` saturating, from the two u32 arrays
    ``DeviceStore.aux_counts`` returns.  The result is ``quant_text_lines``'s."""
    import ctypes as C

    from . import _lib
    from .types import take_text_result

    unique = np.ascontiguousarray(unique, dtype=np.uint32)
    total = np.ascontiguousarray(total, dtype=np.uint32)
    if len(unique) != len(total):
        raise ValueError("ambig_text: unique and total differ in length")
    n = len(unique)
    prefix = bytes(prefix)
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.oem_ambig_text(unique.ctypes.data if n else None, total.ctypes.data if n else None, n,
                                prefix if prefix else None, len(prefix), device, C.byref(h)))
    return take_text_result(L, h, offsets)


def quant_text(names, lens, counts, device: int = 0) -> bytes:
    """The finished `.quant` file (header line and all), its lines formatted on the device."""
    return quant_text_lines(names, lens, counts, _QUANT_HEADER.encode(), device, offsets=False).text.tobytes()


def ambig_text(unique, total, device: int = 0) -> bytes:
    """The finished `.ambig_info.tsv` file (header line and all), its lines formatted on the device."""
    return ambig_text_lines(unique, total, _AMBIG_HEADER.encode(), device, offsets=False).text.tobytes()


def write_output_device(output: str, info: dict, names, lens, counts, aux_counts, device: int = 0) -> None:
    """``write_output`` with the lines of `.quant` and `.ambig_info.tsv` formatted on the device: the same three
    files, byte for byte.  ``aux_counts`` is the pair ``(unique, total)`` that ``DeviceStore.aux_counts`` returns.
    Each text file is one device call and one write."""
    unique, total = aux_counts
    if not (len(lens) == len(counts) == len(unique) == len(total)):
        raise ValueError("write_output_device: per-transcript columns differ in length")
    quant = quant_text_lines(names, lens, counts, _QUANT_HEADER.encode(), device, offsets=False)
    ambig = ambig_text_lines(unique, total, _AMBIG_HEADER.encode(), device, offsets=False)
    _write_meta_info(output, info)
    with open(with_additional_extension(output, ".quant"), "wb") as fh:
        fh.write(quant.text)
    with open(with_additional_extension(output, ".ambig_info.tsv"), "wb") as fh:
        fh.write(ambig.text)


def write_infrep_file(output: str, breps) -> str:
    """bulk.rs:181-193 + parquet_utils.rs:15-44: one non-nullable f64 column `bootstrap.{i}` per
    replicate, one row per transcript; zstd, format v2, plain encoding, statistics on."""
    import pyarrow as pa
    import pyarrow.parquet as pq

    breps = np.asarray(breps, dtype=np.float64)
    if breps.ndim != 2:
        raise ValueError("breps must be n_boot x n_txps")
    fields = [pa.field(f"bootstrap.{i}", pa.float64(), nullable=False) for i in range(breps.shape[0])]
    table = pa.Table.from_arrays([pa.array(np.ascontiguousarray(b)) for b in breps], schema=pa.schema(fields))
    path = with_additional_extension(output, ".infreps.pq")
    _make_parent(output)
    pq.write_table(table, path, compression="zstd", version="2.6", use_dictionary=False,
                   write_statistics=True, data_page_version="2.0")
    return path


def prob_display_decimals(display_thresh: float) -> int:
    """write_function.rs:218-224: ceil(-log10(thresh)) clamped to [3, 9]; 9 for degenerate input."""
    if display_thresh > 0.0 and math.isfinite(display_thresh):
        return int(min(max(math.ceil(-math.log10(display_thresh)), 3.0), 9.0))
    return 9


def write_out_prob(output: str, row_ptr, tid, probs, read_names: Iterable[str], txp_names: Sequence[str],
                   display_thresh: float, compressed: bool = False) -> str:
    """write_function.rs:226-340.  `probs` is what `DeviceStore.assignment_probs(counts,
    display_thresh)` returns: the renormalised probability of every printed alignment, -1 for
    the ones below the threshold (the arithmetic of :283-318 runs on the device)."""
    if compressed:
        raise NotImplementedError(".prob.lz4 needs an lz4 frame encoder, which this image lacks")
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    tid = np.asarray(tid)
    probs = np.asarray(probs, dtype=np.float64)
    d = prob_display_decimals(display_thresh)
    path = with_additional_extension(output, ".prob")
    _make_parent(output)
    with open(path, "w", buffering=1 << 20) as fh:
        fh.write(f"{len(txp_names)}\t{len(row_ptr) - 1}\n")
        for t in txp_names:
            fh.write(f"{t}\n")
        for r, name in enumerate(read_names):
            b, e = row_ptr[r], row_ptr[r + 1]
            keep = probs[b:e] >= 0.0
            ids = tid[b:e][keep]
            pv = probs[b:e][keep]
            fh.write(f"{name.rstrip(chr(0))}\t{len(ids)}\t" + "\t".join(str(int(x)) for x in ids) + "\t"
                     + "\t".join(f"{x:.{d}f}" for x in pv) + "\n")
    return path


def write_out_prob_device(output: str, dev, counts, read_names, txp_names: Sequence[str], display_thresh: float,
                          compressed: bool = False) -> str:
    """write_function.rs:226-340 with the body lines formatted on the device: the header (`T\tR`, the transcript
    names) is written here, then the bytes of ``dev.assignment_text(counts, display_thresh, read_names)`` in one
    write.  The file equals ``write_out_prob``'s byte for byte, with one exception: where every kept alignment of a
    read has probability zero (``display_thresh <= 0`` only), the renormalised values are 0/0; the reference keeps
    those alignments and prints each as `NaN`, and so does the device, while ``write_out_prob`` -- whose ``probs >= 0``
    mask a NaN fails -- prints the read with ``k = 0``.

    ``compressed``: `<out>.prob.lz4` instead, in one write: the LZ4 frame ``dev.assignment_text_lz4`` makes on the
    device of the header lines (its prefix) and the same body; it decodes to the bytes of the uncompressed file."""
    header = f"{len(txp_names)}\t{dev.n_reads}\n".encode() + "".join(f"{t}\n" for t in txp_names).encode()
    _make_parent(output)
    if compressed:
        frame = dev.assignment_text_lz4(counts, display_thresh, read_names, prefix=header)
        path = with_additional_extension(output, ".prob.lz4")
        with open(path, "wb") as fh:
            fh.write(frame.text)
        return path
    body = dev.assignment_text(counts, display_thresh, read_names)
    path = with_additional_extension(output, ".prob")
    with open(path, "wb") as fh:
        fh.write(header)
        fh.write(body.text)
    return path


def cell_triplets(cell_counts) -> tuple:
    """single_cell.rs:155-160: per cell keep v > 0 as f32 -> (row_ids, col_ids, vals) of the
    cells x transcripts count matrix."""
    cell_counts = np.asarray(cell_counts, dtype=np.float64)
    rows, cols = np.nonzero(cell_counts > 0.0)
    return rows.astype(np.uint32), cols.astype(np.uint32), cell_counts[rows, cols].astype(np.float32)


def csr_triplets(indptr, cols, vals) -> tuple:
    """The (row_ids, col_ids, vals) of `cell_triplets` from the CSR form of `em_cells_sparse` (per cell the
    entries v > 0 in ascending column, values already f32): the same triplets in the same order."""
    indptr = np.asarray(indptr, dtype=np.uint64)
    counts = np.diff(indptr.astype(np.int64))
    rows = np.repeat(np.arange(len(counts), dtype=np.uint32), counts)
    return rows, np.asarray(cols, dtype=np.uint32), np.asarray(vals, dtype=np.float32)


_MTX_BANNER = "%%MatrixMarket matrix coordinate real general\n% written by sprs\n"


def cell_barcodes(barcodes, order, cell_rec_off) -> list:
    """The cells' barcodes in result order, for `.barcodes.txt`: cell c's is the barcode of record
    ``order[cell_rec_off[c]]``.  ``barcodes``: one per record in input order, whatever ``types.pack_read_names`` accepts;
    ``order`` / ``cell_rec_off``: what ``em.collate_barcodes`` or ``em_cells_records_sparse(..., barcodes=)`` returned.
    Returns a list of ``str`` (bytes above 0x7f as latin-1), what ``write_single_cell_output*`` take."""
    import numpy as np
    from .types import pack_read_names
    n = len(barcodes[1]) - 1 if isinstance(barcodes, tuple) and len(barcodes) == 2 and not isinstance(barcodes[1], (str, bytes)) else len(barcodes)
    blob, off = pack_read_names(barcodes, n)
    order = np.asarray(order)
    cell_rec_off = np.asarray(cell_rec_off, dtype=np.int64)
    raw = blob.tobytes()
    out = []
    for c in range(len(cell_rec_off) - 1):
        i = int(order[cell_rec_off[c]])
        out.append(raw[int(off[i]):int(off[i + 1])].decode("latin-1"))
    return out


def cell_labels(whitelist, wl_id, order, cell_rec_off) -> list:
    """The cells' barcodes in result order under a whitelist, for `.barcodes.txt`: cell c's is the whitelist's label
    ``wl_id[order[cell_rec_off[c]]]``, never a record's own (raw) bytes.  ``whitelist``: whatever ``types.pack_read_names``
    accepts; ``wl_id`` / ``order`` / ``cell_rec_off``: what ``em.correct_barcodes`` or ``em_cells_records_sparse(...,
    whitelist=)`` returned.  Returns a list of ``str`` as ``cell_barcodes`` does."""
    from .types import pack_read_names
    w = len(whitelist[1]) - 1 if isinstance(whitelist, tuple) and len(whitelist) == 2 and not isinstance(whitelist[1], (str, bytes)) else len(whitelist)
    blob, off = pack_read_names(whitelist, w)
    wl_id, order = np.asarray(wl_id), np.asarray(order)
    cell_rec_off = np.asarray(cell_rec_off, dtype=np.int64)
    raw = blob.tobytes()
    out = []
    for c in range(len(cell_rec_off) - 1):
        label = int(wl_id[int(order[cell_rec_off[c]])])
        if label >= w:
            raise ValueError(f"cell {c}: its first record has no label")
        out.append(raw[int(off[label]):int(off[label + 1])].decode("latin-1"))
    return out


def _write_single_cell_side_files(output: str, info: dict, feature_names: Sequence[str],
                                  barcodes: Optional[Sequence[str]]) -> None:
    """What a single-cell run writes besides the matrix: `.meta_info.json`, `.features.txt` and, in row order,
    `.barcodes.txt` (write_function.rs:25-69, single_cell.rs:176-178)."""
    _make_parent(output)
    with open(with_additional_extension(output, ".meta_info.json"), "w") as fh:
        json.dump(info, fh, indent=2)
    with open(with_additional_extension(output, ".features.txt"), "w") as fh:
        for n in feature_names:
            fh.write(f"{n}\n")
    if barcodes is not None:
        with open(with_additional_extension(output, ".barcodes.txt"), "w") as fh:
            for b in barcodes:
                fh.write(f"{b}\n")


def write_single_cell_output(output: str, info: dict, feature_names: Sequence[str], barcodes: Optional[Sequence[str]],
                             n_cells: int, row_ids, col_ids, vals) -> None:
    """write_function.rs:25-69: `.meta_info.json`, `.count.mtx` (MatrixMarket coordinate real
    general, 1-based, f32 values in triplet order as sprs::io::write_matrix_market emits them) and
    `.features.txt`; `.barcodes.txt` in row order (single_cell.rs:176-178).  The triplets come from
    `cell_triplets(dense)` or `csr_triplets(*em_cells_sparse(...)[:3])`."""
    _write_single_cell_side_files(output, info, feature_names, barcodes)
    with open(with_additional_extension(output, ".count.mtx"), "w") as fh:
        fh.write(_MTX_BANNER)
        fh.write(f"{int(n_cells)} {len(feature_names)} {len(vals)}\n")
        for r, c, v in zip(row_ids, col_ids, vals):
            fh.write(f"{int(r) + 1} {int(c) + 1} {rust_display(v, f32=True)}\n")


def write_single_cell_output_device(output: str, info: dict, feature_names: Sequence[str],
                                    barcodes: Optional[Sequence[str]], n_cells: int, indptr, cols, vals,
                                    device: int = 0) -> None:
    """``write_single_cell_output`` with the matrix lines formatted on the device: the same four files, byte for
    byte, from the CSR ``em_cells_sparse`` returns (no triplets are built).  `.count.mtx` is the text of
    ``em.count_matrix_text`` -- the banner and the dimension line go in as its prefix -- written in one write."""
    from .em import count_matrix_text

    if len(indptr) != int(n_cells) + 1:
        raise ValueError("indptr must hold n_cells + 1 offsets")
    _write_single_cell_side_files(output, info, feature_names, barcodes)
    prefix = (_MTX_BANNER + f"{int(n_cells)} {len(feature_names)} {len(vals)}\n").encode()
    body = count_matrix_text(indptr, cols, vals, len(feature_names), prefix=prefix, device=device, offsets=False)
    with open(with_additional_extension(output, ".count.mtx"), "wb") as fh:
        fh.write(body.text)


def write_single_cell_gene_output_device(output: str, gene_names: Sequence[str], n_cells: int, indptr_g, genes, vals_g,
                                         device: int = 0) -> None:
    """The gene-level matrix beside `.count.mtx`, from the CSR ``em.cells_gene_counts`` returns: `.gene_count.mtx`
    (cells x genes, the text of ``em.count_matrix_text`` with the banner and the dimension line as its prefix: the
    format of `.count.mtx`, formatted by the same kernel) and `.gene_features.txt`, one gene name per line in gene-id
    order."""
    from .em import count_matrix_text

    if len(indptr_g) != int(n_cells) + 1:
        raise ValueError("indptr_g must hold n_cells + 1 offsets")
    _make_parent(output)
    prefix = (_MTX_BANNER + f"{int(n_cells)} {len(gene_names)} {len(vals_g)}\n").encode()
    body = count_matrix_text(indptr_g, genes, vals_g, len(gene_names), prefix=prefix, device=device, offsets=False)
    with open(with_additional_extension(output, ".gene_count.mtx"), "wb") as fh:
        fh.write(body.text)
    with open(with_additional_extension(output, ".gene_features.txt"), "w") as fh:
        for n in gene_names:
            fh.write(f"{n}\n")
