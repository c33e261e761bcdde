"""The tail of the reference's bulk driver, on the device engine:
`perform_inference_and_write_output` (src/bulk.rs:82-209) from the built store onwards --
EMInfo assembly, `em` / `em_par` by thread count (:155-159), aux counts (:161), `.quant` /
`.ambig_info.tsv` / `.meta_info.json` (:168-174), bootstraps -> `.infreps.pq` (:178-193),
assignment probabilities -> `.prob` (:196-207).  With a `BulkCoverage`, the driver also runs the coverage
model of :103-108 (`logistic_prob` + `normalize_read_probs` when `model_coverage` is set) first, on the device
and in the same call that creates the resident store (`InMemoryAlignmentStore.model_coverage_on_device`).
Alignment parsing comes before this (the caller); the filtering is `builder.StoreBuilder` (one read or a batch of
reads per call, on the host or on the device) or, from the parsed records straight to the resident store in one device
call, `DeviceStore.from_records` (oem_store_create_records).  `quantify_bulk_alignments_from_records` is the whole of
`quantify_bulk_alignments_from_bam` (bulk.rs:212-259) from the parsed records on: the parser itself
(alignment_parser.rs:301-437) runs on the device too (`DeviceStore.from_named_records`);
`quantify_bulk_alignments_from_record_batches` is the same for a reader that hands the records and names over in chunks
(`builder.RecordsStream(names=True)`).  Genome mode has the same pair from the projected groups on
(`quantify_genome_alignments_from_bam`, bulk.rs:268-335): `quantify_genome_alignments_from_projected_records`
(`DeviceStore.from_projected_records`) and `quantify_genome_alignments_from_projected_batches`
(`builder.RecordsStream(projected=True)`).  KDE is not supported.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from . import writers
from .em import bootstrap, em, em_par
from .types import DeviceStore, EMInfo, InMemoryAlignmentStore, TranscriptInfo


def read_short_quant_vec(short_read_path: str, txps_name: Sequence[str]) -> np.ndarray:
    """`--short-quant` (util/read_function.rs:9-85): a salmon-style `quant.sf` TSV (columns Name, Length,
    EffectiveLength, TPM, NumReads) projected onto the transcript order of the header -> the EM's
    `init_abundances` (bulk.rs:118-120).  A name in the file that the header lacks is an error; a
    header transcript missing from the file gets 0."""
    import csv
    with open(short_read_path, newline="") as fh:
        rdr = csv.DictReader(fh, delimiter="\t")
        need = {"Name", "Length", "EffectiveLength", "TPM", "NumReads"}
        if rdr.fieldnames is None or not need.issubset(rdr.fieldnames):
            raise ValueError(f"{short_read_path}: expected the columns {sorted(need)}")
        records = {}
        for rec in rdr:
            int(rec["Length"]); float(rec["EffectiveLength"]); float(rec["TPM"])   # deserialised (and checked) as in the reference
            records[rec["Name"]] = float(rec["NumReads"])
    names = set(txps_name)
    if not all(k in names for k in records):
        raise ValueError("There were transcripts in the short read quantification file that didn't appear in "
                         "the BAM header; cannot proceed.")
    return np.array([records.get(n, 0.0) for n in txps_name], dtype=np.float64)


@dataclass
class BulkCoverage:
    """`--model-coverage` (prog_opts.rs) for the bulk driver: the alignments' coordinates (AlnInfo start / end, one
    entry per alignment of the store, in its order) and the model's `--bin-width` / `--growth-rate`."""
    aln_start: np.ndarray
    aln_end: np.ndarray
    bin_width: int = 100                  # prog_opts.rs:555
    growth_rate: float = 2.0              # prog_opts.rs:502


@dataclass
class BulkArgs:
    """The `Args` fields this stage reads (prog_opts.rs): defaults are the reference's."""
    output: str
    threads: int = 3                      # prog_opts.rs:543
    max_em_iter: int = 1000               # :532
    convergence_thresh: float = 1e-3      # :536
    num_bootstraps: int = 0
    write_assignment_probs: bool = False
    display_thresh: float = 1e-6
    prob_on_device: bool = False          # `.prob` body formatted on the device (writers.write_out_prob_device)
    prob_compressed: bool = False         # `--write-assignment-probs=compressed` (prog_opts.rs:506-513): `.prob.lz4`; on the device with prob_on_device
    quant_on_device: bool = False         # `.quant` and `.ambig_info.tsv` lines formatted on the device (writers.write_output_device)
    seed: int = 0                         # the reference seeds from the OS (em.rs:274)
    device: int = 0
    extra_info: dict = field(default_factory=dict)


def perform_inference_and_write_output(store: InMemoryAlignmentStore, txps_name: Sequence[str],
                                       txp_lens: Sequence[int], args: BulkArgs,
                                       init_abundances: Optional[np.ndarray] = None,
                                       read_names: Optional[Sequence[str]] = None,
                                       coverage: Optional[BulkCoverage] = None) -> np.ndarray:
    if coverage is not None:                                                             # bulk.rs:103-108
        store.model_coverage_on_device(coverage.aln_start, coverage.aln_end, np.asarray(txp_lens, dtype=np.uint64),
                                       coverage.bin_width, coverage.growth_rate, device=args.device)
    txps = [TranscriptInfo.with_len(int(l)) for l in txp_lens]
    emi = EMInfo(eq_map=store, txp_info=txps, max_iter=args.max_em_iter,
                 convergence_thresh=args.convergence_thresh, init_abundances=init_abundances,
                 device=args.device)
    counts = em_par(emi, args.threads) if args.threads > 4 else em(emi, args.threads)   # bulk.rs:155-159
    dev = store.device_store(len(txps), args.device)
    unique, total = dev.aux_counts()                                                     # bulk.rs:161
    info = {"num_aligned_reads": store.num_aligned_reads(), "total_alignments": store.total_len(),
            "em_max_iter": args.max_em_iter, "em_convergence_thresh": args.convergence_thresh,
            "threads": args.threads, "num_bootstraps": args.num_bootstraps, "output": args.output,
            "filter_options": {"model_coverage": store.filter_opts.model_coverage},
            "em_iterations": emi.last_run_info.niter if emi.last_run_info else None}
    info.update(args.extra_info)
    if args.quant_on_device:                                                             # bulk.rs:168-174
        writers.write_output_device(args.output, info, txps_name, txp_lens, counts, (unique, total), device=args.device)
    else:
        writers.write_output(args.output, info, txps_name, txp_lens, counts, unique, total)
    if args.num_bootstraps > 0:                                                          # bulk.rs:178-193
        breps = bootstrap(emi, args.num_bootstraps, args.threads, seed=args.seed)
        writers.write_infrep_file(args.output, breps)
    if args.write_assignment_probs:                                                      # bulk.rs:196-207
        if read_names is None:
            raise ValueError("cannot write assignment probabilities without valid vector of read names")
        if args.prob_on_device:
            writers.write_out_prob_device(args.output, dev, counts, read_names, txps_name, args.display_thresh,
                                          compressed=args.prob_compressed)
            return counts
        probs = dev.assignment_probs(counts, args.display_thresh)
        writers.write_out_prob(args.output, store.boundaries, store.alignments, probs, read_names, txps_name,
                               args.display_thresh, compressed=args.prob_compressed)
    return counts


def quantify_bulk_alignments_from_records(filters, txps_name: Sequence[str], txp_lens: Sequence[int], records, names,
                                          args: BulkArgs, secondary=None, mode: str = "adjacent",
                                          sort_check_num: int = 100_000, coverage: Optional[str] = None,
                                          bin_width: int = 100, growth_rate: float = 2.0) -> np.ndarray:
    """`quantify_bulk_alignments_from_bam` (bulk.rs:212-259) from the parsed records on: ``records``, their read
    ``names`` and ``secondary`` flags in input order go through ``DeviceStore.from_named_records`` (the parser of
    alignment_parser.rs:301-437, the filter and, with ``coverage`` "logistic" / "binomial", the coverage model of
    bulk.rs:103-108, in one device call), then the tail of ``perform_inference_and_write_output``: the EM by thread count
    (:155-159), aux counts, `.quant` / `.ambig_info.tsv` / `.meta_info.json`, bootstraps, and `.prob` with the read names
    the parser collected.  The files are those of ``perform_inference_and_write_output`` on the store the host builder
    makes of the same groups.  The resident store has no host CSR, so the host `.prob` writer (``prob_on_device``
    False) first runs the host filter once more over the collated records for the rows' transcript ids;
    ``prob_on_device`` formats the body from the resident store and needs none of that."""
    txp_len = np.asarray(txp_lens, dtype=np.uint64)
    dev, _kept, _discard, parse = DeviceStore.from_named_records(
        filters, txp_len, records, names, secondary=secondary, mode=mode, sort_check_num=sort_check_num, coverage=coverage,
        bin_width=bin_width, growth_rate=growth_rate, device=args.device)
    return _write_from_resident(dev, parse, lambda: (np.asarray(records)[parse.order], parse.group_off), filters, txp_len,
                                txps_name, txp_lens, args, coverage)


def quantify_bulk_alignments_from_record_batches(filters, txps_name: Sequence[str], txp_lens: Sequence[int], batches,
                                                 args: BulkArgs, sort_check_num: int = 100_000,
                                                 coverage: Optional[str] = None, bin_width: int = 100,
                                                 growth_rate: float = 2.0, max_staged_records: int = 0,
                                                 mode: str = "adjacent") -> np.ndarray:
    """``quantify_bulk_alignments_from_records`` for a reader that hands over chunks: ``batches`` is an iterable of
    ``(records, names)`` in input order, cut at any record positions (a read may straddle batches).  They go through a
    names session (``RecordsStream(names=True)``: the reference's parser, ``mode="adjacent"``); the files are those of
    ``quantify_bulk_alignments_from_records`` on the concatenation.  The host `.prob` writer (``prob_on_device`` False)
    keeps the mapped records it has seen for the rows' transcript ids; ``prob_on_device`` needs none of that.

    ``mode="sort"`` takes ``(records, names[, secondary])`` batches in ANY order -- a coordinate-sorted or unsorted
    input -- through a sorting names session (``RecordsStream(names=True, mode="sort")``); the files are those of
    ``quantify_bulk_alignments_from_records(mode="sort")`` on the concatenation.  ``sort_check_num`` is not read then.
    The host `.prob` writer keeps every record it has seen, ``parse.order`` indexing all of them."""
    from .builder import ALN_RECORD, REC_UNMAPPED, RecordsStream
    if mode not in ("adjacent", "sort"):
        raise ValueError(f"mode must be 'adjacent' or 'sort', not {mode!r}")
    sorting = mode == "sort"
    txp_len = np.asarray(txp_lens, dtype=np.uint64)
    keep_rows = args.write_assignment_probs and not args.prob_on_device
    mapped = []
    with RecordsStream(filters, txp_len, coverage=coverage, bin_width=bin_width, growth_rate=growth_rate, device=args.device,
                       max_staged_records=max_staged_records, names=True, sort_check_num=sort_check_num, mode=mode) as rs:
        for batch in batches:
            if len(batch) != 2 and not (sorting and len(batch) == 3):
                raise ValueError("a batch is (records, names)" + (" or (records, names, secondary)" if sorting else ""))
            records = np.asarray(batch[0])
            if sorting:
                rs.push(records, names=batch[1], secondary=batch[2] if len(batch) == 3 else None)
            else:
                rs.push(records, names=batch[1])
            if keep_rows:
                mapped.append(records if sorting else records[(records["flags"] & REC_UNMAPPED) == 0])
        dev, _kept, _discard, parse = rs.finish()

    def host_rows():
        seen = np.concatenate(mapped) if mapped else np.zeros(0, dtype=ALN_RECORD)
        return (seen[parse.order] if sorting else seen), parse.group_off

    return _write_from_resident(dev, parse, host_rows, filters, txp_len, txps_name, txp_lens, args, coverage)


def _projected_batch(batch):
    """One ``(records, group_off, read_len[, read_names[, genomic_counts]])`` of the genome-mode drivers, checked: the
    arrays, the groups' names as a list (or None) and the genomic record counts (or None)."""
    from .builder import check_projected_batch
    if not 3 <= len(batch) <= 5:
        raise ValueError("a projected batch is (records, group_off, read_len[, read_names[, genomic_counts]])")
    records, group_off, read_len = check_projected_batch(*batch[:3])
    n_groups = len(group_off) - 1
    names = None if len(batch) < 4 or batch[3] is None else list(batch[3])
    if names is not None and len(names) != n_groups:
        raise ValueError("read_names must have one entry per group")
    counts = None if len(batch) < 5 or batch[4] is None else np.asarray(batch[4], dtype=np.int64)
    if counts is not None and counts.shape != (n_groups,):
        raise ValueError("genomic_counts must have one entry per group")
    return records, group_off, read_len, names, counts


def _projected_tail(dev, kept, pieces, filters, txp_len, txps_name, txp_lens, args: BulkArgs, beta, prob_source, coverage):
    """What both genome-mode drivers do once the store stands: ``unique_alignments`` (alignment_parser.rs:654-657: a kept
    group that was projected from one genomic record), the kept groups' names (:620-630) and the shared tail."""
    from types import SimpleNamespace
    from .builder import PROJ_RECORD
    from .types import pack_read_names
    names, counts = [], []
    for _, _, _, nm, cnt in pieces:
        names.append(nm)
        counts.append(cnt)
    unique = None
    if all(c is not None for c in counts):
        genomic = np.concatenate(counts) if counts else np.zeros(0, dtype=np.int64)
        unique = int(np.count_nonzero((kept > 0) & (genomic == 1)))
    read_names = None
    if args.write_assignment_probs:
        if any(n is None for n in names):
            raise ValueError("cannot write assignment probabilities without valid vector of read names")
        flat = [n for nm in names for n in nm]
        rows = [flat[g] for g in np.flatnonzero(kept)]
        read_names = pack_read_names(rows, len(rows))

    def host_rows():   # (the host `.prob` writer alone: the groups once more, concatenated)
        off, base = [np.zeros(1, dtype=np.uint64)], 0
        for _, group_off, _, _, _ in pieces:
            off.append(group_off[1:] + np.uint64(base))
            base += int(group_off[-1])
        recs = [p[0] for p in pieces]
        return (np.concatenate(recs) if recs else np.zeros(0, dtype=PROJ_RECORD), np.concatenate(off),
                np.concatenate([p[2] for p in pieces]) if pieces else np.zeros(0, dtype=np.uint64))

    parse = SimpleNamespace(read_names=read_names)
    counts_out = _write_from_resident(dev, parse, host_rows, filters, txp_len, txps_name, txp_lens, args, coverage,
                                      projected=(beta, prob_source))
    return counts_out, unique


def quantify_genome_alignments_from_projected_records(filters, txps_name: Sequence[str], txp_lens: Sequence[int], records,
                                                      group_off, read_len, args: BulkArgs, read_names=None,
                                                      genomic_counts=None, beta: float = 10.0, prob_source="similarity",
                                                      coverage: Optional[str] = None, bin_width: int = 100,
                                                      growth_rate: float = 2.0):
    """`quantify_genome_alignments_from_bam` (bulk.rs:268-335) from the projected groups on: the reads' projected
    ``records`` (``builder.PROJ_RECORD``) with ``group_off`` and ``read_len`` go through
    ``DeviceStore.from_projected_records`` (filter_projected and, with ``coverage``, the model of bulk.rs:103-108, in one
    device call), then the tail of ``perform_inference_and_write_output``.  ``read_names``: one name per group, needed
    for `.prob`, whose rows are the kept groups' names (alignment_parser.rs:620-630).  ``genomic_counts``: the number of
    genomic records each group was projected from.  Returns ``(counts, unique_alignments)``: the groups with
    ``kept > 0`` and ``genomic_counts == 1`` (:654-657), None without ``genomic_counts``.  The files are those of
    ``perform_inference_and_write_output`` on the store the host builder makes of the same groups
    (``StoreBuilder.add_projected_groups``)."""
    txp_len = np.asarray(txp_lens, dtype=np.uint64)
    piece = _projected_batch((records, group_off, read_len, read_names, genomic_counts))
    dev, kept, _discard = DeviceStore.from_projected_records(filters, txp_len, piece[0], piece[1], piece[2], beta=beta,
                                                             prob_source=prob_source, coverage=coverage, bin_width=bin_width,
                                                             growth_rate=growth_rate, device=args.device)
    return _projected_tail(dev, kept, [piece], filters, txp_len, txps_name, txp_lens, args, beta, prob_source, coverage)


def quantify_genome_alignments_from_projected_batches(filters, txps_name: Sequence[str], txp_lens: Sequence[int], batches,
                                                      args: BulkArgs, beta: float = 10.0, prob_source="similarity",
                                                      coverage: Optional[str] = None, bin_width: int = 100,
                                                      growth_rate: float = 2.0, max_staged_records: int = 0):
    """``quantify_genome_alignments_from_projected_records`` for a driver that projects reads as they come
    (parse_genome_alignments, alignment_parser.rs:580-700; the mapper threads of quantify_genome_raw_reads,
    bulk.rs:337-682): ``batches`` is an iterable of ``(records, group_off, read_len[, read_names[, genomic_counts]])``,
    whole groups each, ``group_off`` from 0.  They go through a projected session
    (``RecordsStream(projected=True)``); the files and the returned ``(counts, unique_alignments)`` are those of the
    one-call form on the concatenation.  Only the host `.prob` writer (``prob_on_device`` False) keeps the records it has
    seen; names and genomic counts are kept per group."""
    from .builder import RecordsStream
    txp_len = np.asarray(txp_lens, dtype=np.uint64)
    keep_rows = args.write_assignment_probs and not args.prob_on_device
    pieces = []
    with RecordsStream(filters, txp_len, coverage=coverage, bin_width=bin_width, growth_rate=growth_rate, device=args.device,
                       max_staged_records=max_staged_records, projected=True, beta=beta, prob_source=prob_source) as rs:
        for batch in batches:
            records, group_off, read_len, names, counts = _projected_batch(batch)
            rs.push(records, group_off, read_len=read_len)
            pieces.append((records, group_off, read_len, names, counts) if keep_rows else (None, None, None, names, counts))
        dev, kept, _discard = rs.finish()
    return _projected_tail(dev, kept, pieces, filters, txp_len, txps_name, txp_lens, args, beta, prob_source, coverage)


def _write_from_resident(dev, parse, host_rows, filters, txp_len, txps_name, txp_lens, args: BulkArgs, coverage,
                         projected=None) -> np.ndarray:
    """The tail the records drivers share, from the resident store on.  ``host_rows()``: the collated records and their
    group_off for the host `.prob` writer, which needs the rows' transcript ids; with ``projected`` = (beta,
    prob_source) they are projected records, ``host_rows()`` gives their read lengths too and the host filter is
    ``add_projected_groups``."""
    from .builder import StoreBuilder
    with dev:
        counts, run = dev.em_run(None, args.max_em_iter, args.convergence_thresh, 50 if args.threads <= 4 else 1)  # bulk.rs:155-159
        unique, total = dev.aux_counts()                                                     # bulk.rs:161
        info = {"num_aligned_reads": dev.n_reads, "total_alignments": dev.nnz,
                "em_max_iter": args.max_em_iter, "em_convergence_thresh": args.convergence_thresh,
                "threads": args.threads, "num_bootstraps": args.num_bootstraps, "output": args.output,
                "filter_options": {"model_coverage": coverage is not None},
                "em_iterations": run.niter}
        info.update(args.extra_info)
        if args.quant_on_device:                                                             # bulk.rs:168-174
            writers.write_output_device(args.output, info, txps_name, txp_lens, counts, (unique, total), device=args.device)
        else:
            writers.write_output(args.output, info, txps_name, txp_lens, counts, unique, total)
        if args.num_bootstraps > 0:                                                          # bulk.rs:178-193
            breps, _ = dev.bootstrap(args.num_bootstraps, args.seed, None, None, args.max_em_iter, args.convergence_thresh)
            writers.write_infrep_file(args.output, [breps[b] for b in range(args.num_bootstraps)])
        if args.write_assignment_probs:                                                      # bulk.rs:196-207
            if args.prob_on_device:
                writers.write_out_prob_device(args.output, dev, counts, parse.read_names, txps_name, args.display_thresh,
                                              compressed=args.prob_compressed)
                return counts
            with StoreBuilder(filters, txp_len) as hb:   # the rows' transcript ids: the host filter over the same groups
                if projected is None:
                    hb.add_groups(*host_rows())
                else:
                    hb.add_projected_groups(*host_rows(), beta=projected[0], prob_source=projected[1])
                row_ptr, tid = hb.export()[:2]
            blob, off = parse.read_names
            read_names = [bytes(blob[int(off[r]):int(off[r + 1])]).decode("utf-8", "replace") for r in range(dev.n_reads)]
            probs = dev.assignment_probs(counts, args.display_thresh)
            writers.write_out_prob(args.output, row_ptr, tid, probs, read_names, txps_name, args.display_thresh,
                                   compressed=args.prob_compressed)
    return counts
