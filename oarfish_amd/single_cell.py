"""The single-cell driver (src/single_cell.rs:54-290 of COMBINE-lab/oarfish) from the parsed records on.

The reference walks a barcode-collated BAM record by record, cuts a cell where the ``CB`` tag changes
(single_cell.rs:196-227, alignment_parser.rs:244-299), hands every cell to a worker -- sort by read name, filter,
coverage model, EM, the entries above 0 (:104-188) -- and writes the matrix with its side files (:259).  Here the
reader's batches go into a barcoded session (``CellsStream(barcodes=True)``): the cut, the collation, the filter and the
EM run on the device while the reader goes on, and nothing run-sized is held on the host.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from . import writers
from .em import CellsStream, _n_packed


@dataclass
class SingleCellArgs:
    """The `Args` fields this stage reads (prog_opts.rs): defaults are the reference's."""
    output: str
    threads: int = 3
    max_em_iter: int = 1000
    convergence_thresh: float = 1e-3
    model_coverage: Optional[str] = None   # None, "binomial" or "logistic"
    bin_width: int = 100
    growth_rate: float = 2.0
    mode: str = "sort"                     # the reference sorts every cell by read name; "adjacent": name-collated cells
    device: int = 0
    group_nnz: int = 0                     # the session's budgets, 0 = the library's defaults
    group_cells: int = 0
    max_staged_records: int = 0
    collated: bool = True                  # False: the batches' records come in any order (the any-order barcoded session)
    umis: bool = False                     # True: the batches carry a UMI per record and every cell is deduplicated
    gene_of: Optional[Sequence[int]] = None     # one gene id per transcript: with umis the molecules' keys, with gene_counts the collapse
    gene_names: Optional[Sequence[str]] = None  # one name per gene id, for `.gene_features.txt`
    umi_correct: bool = False              # with umis: UMIs one mismatch from a more abundant one are corrected to it
    gene_counts: bool = False              # True: `.gene_count.mtx` and `.gene_features.txt` beside `.count.mtx`
    whitelist: Optional[Sequence[bytes]] = None  # the batches' barcodes are raw (CR): corrected against these labels (collated=False)
    barcode_multi: bool = False            # with whitelist: of several neighbours the one with strictly the most exact records wins
    extra_info: dict = field(default_factory=dict)

    def __post_init__(self):
        if self.whitelist is not None and self.collated:
            raise ValueError("whitelist requires collated=False: only the any-order barcoded session corrects raw barcodes")
        if self.whitelist is None and self.barcode_multi:
            raise ValueError("barcode_multi goes with whitelist")


def quantify_single_cell_from_record_batches(filters, txps_name: Sequence[str], txp_lens: Sequence[int], batches,
                                             args: SingleCellArgs):
    """``get_single_cell_abundances`` for a reader that hands over chunks: ``batches`` is an iterable of ``(records,
    barcodes, names, secondary)`` in input order (``synth.cut_cell_records``' tuples), barcode-collated and cut at any
    record positions -- or, with ``args.collated=False``, in any order at all (``synth.cut_interleaved_records``' tuples:
    the any-order barcoded session, whose cells are those of the one barcodes call).  Writes `.count.mtx`, `.features.txt`, `.barcodes.txt` (the session's labels, in cell order) and
    `.meta_info.json` with ``writers.write_single_cell_output_device`` and returns ``(indptr, cols, vals, infos,
    cells)``: the session's result and its ``cells()``.

    With ``args.umis`` the batches are 5-tuples ``(records, barcodes, names, secondary, umis)`` (the cutters' tuples under
    ``umis=``), the session deduplicates every cell on the device, ``cells`` carries ``cell_dups`` and `.meta_info.json`
    gains ``umi_dedup`` and ``umi_duplicate_reads``.

    ``args.gene_of`` means one thing end to end.  With ``args.umis`` it goes to the session with ``args.umi_correct`` (the
    UMI rule of ``CellsStream``): `.meta_info.json` gains ``umi_gene_keys`` and ``umi_correct`` and, with correction,
    ``umi_corrected_reads``; ``cells`` carries ``cell_corrected``.  With ``args.gene_counts`` the session's matrix is
    collapsed to cells x genes on the device (``em.cells_gene_counts``) and written as `.gene_count.mtx` with
    `.gene_features.txt` (``writers.write_single_cell_gene_output_device``); ``args.gene_names`` names the genes,
    `.meta_info.json` gains ``gene_counts`` and ``n_genes``, and ``cells`` gains ``gene_counts = (indptr_g, genes,
    vals_g)``.

    With ``args.whitelist`` (and ``args.collated=False``) the batches' barcodes are raw and the session corrects them
    against the whitelist (``CellsStream(..., whitelist=, barcode_multi=)``): `.barcodes.txt` gets the whitelist's labels,
    never a record's raw bytes, `.meta_info.json` gains ``barcode_whitelist_labels``, ``barcode_multi`` and the five counts
    (``barcode_exact``, ``barcode_corrected``, ``barcode_no_neighbour``, ``barcode_ambiguous``, ``barcode_missing``), and
    ``cells`` carries ``cell_wl_id``, ``cell_bc_corrected`` and ``counts``."""
    txp_len = np.asarray(txp_lens, dtype=np.uint64)
    gene_of = None if args.gene_of is None else np.asarray(args.gene_of)
    if gene_of is not None and (gene_of.ndim != 1 or len(gene_of) != len(txp_len)):
        raise ValueError("gene_of must hold one gene id per transcript")
    if args.umi_correct and not args.umis:
        raise ValueError("umi_correct goes with umis: it is part of the rule the UMIs are deduplicated by")
    if gene_of is not None and not (args.umis or args.gene_counts):
        raise ValueError("gene_of goes with umis (the molecules' keys) or gene_counts (the collapse)")
    if args.gene_counts:
        if gene_of is None or args.gene_names is None:
            raise ValueError("gene_counts needs gene_of and gene_names")
        if not len(gene_of) or int(gene_of.min()) < 0:
            raise ValueError("gene_of must hold gene ids from 0")
        n_genes = int(gene_of.max()) + 1
        if len(args.gene_names) != n_genes:
            raise ValueError(f"gene_names must name the {n_genes} genes of gene_of, not {len(args.gene_names)}")
    rule = dict(gene_of=gene_of, umi_correct=args.umi_correct) if args.umis else {}
    if args.whitelist is not None:
        rule.update(whitelist=args.whitelist, barcode_multi=args.barcode_multi)
    coverage = None
    if args.model_coverage is not None:
        coverage = dict(model=args.model_coverage, bin_width=args.bin_width, growth_rate=args.growth_rate, txp_len=txp_len)
    with CellsStream(len(txp_len), max_iter=args.max_em_iter, conv_thresh=args.convergence_thresh, coverage=coverage,
                     device=args.device, group_nnz=args.group_nnz, group_cells=args.group_cells,
                     max_staged_nnz=args.max_staged_records, filters=filters, txp_len=txp_len, barcodes=True,
                     mode=args.mode, collated=args.collated, umis=args.umis, **rule) as cs:
        if args.umis:
            for records, barcodes, names, secondary, umis in batches:
                cs.push_batch(records, barcodes, names, secondary, umis)
        else:
            for records, barcodes, names, secondary in batches:
                cs.push_batch(records, barcodes, names, secondary)
        indptr, cols, vals, infos = cs.finish()
        cells = cs.cells()
    info = {"output": args.output, "single_cell": True, "em_max_iter": args.max_em_iter,
            "em_convergence_thresh": args.convergence_thresh, "threads": args.threads,
            "filter_options": {"model_coverage": args.model_coverage is not None}}
    if args.umis:
        info["umi_dedup"] = True
        info["umi_duplicate_reads"] = int(cells["cell_dups"].sum())
        if gene_of is not None or args.umi_correct:
            info["umi_gene_keys"] = gene_of is not None
            info["umi_correct"] = bool(args.umi_correct)
        if args.umi_correct:
            info["umi_corrected_reads"] = int(cells["cell_corrected"].sum())
    if args.whitelist is not None:
        info["barcode_whitelist_labels"] = _n_packed(args.whitelist)
        info["barcode_multi"] = bool(args.barcode_multi)
        for k, word in enumerate(("exact", "corrected", "no_neighbour", "ambiguous", "missing")):
            info["barcode_" + word] = int(cells["counts"][k])
    if args.gene_counts:
        info["gene_counts"] = True
        info["n_genes"] = n_genes
    info.update(args.extra_info)
    labels = [b.decode("latin-1") for b in cells["barcodes"]]
    writers.write_single_cell_output_device(args.output, info, txps_name, labels, len(labels), indptr, cols, vals,
                                            device=args.device)
    if args.gene_counts:
        from .em import cells_gene_counts
        indptr_g, genes, vals_g = cells_gene_counts(indptr, cols, vals, gene_of, n_genes=n_genes, device=args.device)
        writers.write_single_cell_gene_output_device(args.output, args.gene_names, len(labels), indptr_g, genes, vals_g, device=args.device)
        cells["gene_counts"] = (indptr_g, genes, vals_g)
    return indptr, cols, vals, infos, cells
