"""oarfish_amd -- MI355X-native EM quantification engine for oarfish's hot path.

Only what the path needs: ``csrc/`` (HIP kernels + the C ABI of
``include/oarfish_em.h``), the ctypes loader, and a host-side mirror of the
reference interface (``InMemoryAlignmentStore``, ``EMInfo``, ``em``, ``em_par``,
``bootstrap``; src/em.rs, src/util/oarfish_types.rs of COMBINE-lab/oarfish).
There is no CPU fallback: without ``liboarfish_em.so`` imports of the compute
path fail, and without a HIP device every compute call raises ``OemError``.
"""
from ._lib import OemError, device_count  # noqa: F401
from .types import (AlignmentFilters, DeviceStore, EMInfo, InMemoryAlignmentStore,  # noqa: F401
                    RunInfo, TranscriptInfo)
from .em import (CellsStream, bootstrap, cells_coverage_probs, cells_gene_counts, collate_barcodes, correct_barcodes, collate_names, dedup_umis, dedup_umis_rule, drop_groups, em, em_cells, em_cells_coverage_sparse, em_cells_records_sparse,  # noqa: F401
                 em_cells_sparse,
                 em_par, history_log_records)
from .single_cell import quantify_single_cell_from_record_batches  # noqa: F401
from .synth import add_barcode_errors, add_umi_duplicates, add_umi_errors, make_whitelist, gene_of_txps, cut_cell_records, cut_interleaved_records  # noqa: F401

__all__ = [
    "CellsStream", "AlignmentFilters", "DeviceStore", "EMInfo", "InMemoryAlignmentStore", "RunInfo",
    "TranscriptInfo", "bootstrap", "cells_coverage_probs", "collate_barcodes", "collate_names", "em", "em_cells", "em_cells_coverage_sparse", "em_cells_records_sparse", "em_cells_sparse", "em_par", "history_log_records", "OemError", "device_count",
    "cut_cell_records", "cut_interleaved_records", "quantify_single_cell_from_record_batches",
    "dedup_umis", "drop_groups", "add_umi_duplicates", "dedup_umis_rule", "add_umi_errors", "gene_of_txps",
    "cells_gene_counts", "correct_barcodes", "add_barcode_errors", "make_whitelist",
]
