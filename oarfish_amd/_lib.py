"""ctypes loader of liboarfish_em.so (the C ABI of include/oarfish_em.h).

There is no Python or CPU fallback: if the shared library is missing the import
of the product path fails loudly, and every compute entry point of the library
returns OEM_ERR_NO_DEVICE when no HIP device is present.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "liboarfish_em.so")

OEM_OK = 0
OEM_ERR_ARG = 1
OEM_ERR_OOM = 2
OEM_ERR_HIP = 3
OEM_ERR_RCCL = 4
OEM_ERR_NO_DEVICE = 5
OEM_ERR_STATE = 6
OEM_UNIQUE_ID_BYTES = 128
OEM_P2P_HANDLE_BYTES = 128
OEM_OPT_BATCH_BOOTSTRAP = 1
OEM_OPT_BOOTSTRAP_FIRST_REPLICA = 2
OEM_OPT_RUN_HISTORY = 3
OEM_COMM_OPT_P2P_MAX_BYTES = 1
OEM_COMM_OPT_P2P_SHAPE = 2
OEM_COMM_OPT_P2P_TIMEOUT_MS = 3
OEM_COMM_OPT_P2P_SELF_CHECK = 4
OEM_COMM_INFO_RANKS = 1
OEM_COMM_INFO_RCCL_RANKS = 2
OEM_COMM_INFO_P2P_CONNECTED = 3
OEM_CELLS_STREAM_INFO_CELLS = 1
OEM_CELLS_STREAM_INFO_ALIGNMENTS = 2
OEM_CELLS_STREAM_INFO_GROUPS = 3
OEM_CELLS_STREAM_INFO_GROUPS_BEFORE_FINISH = 4
OEM_CELLS_STREAM_INFO_BLOCKED_US = 5
OEM_CELLS_STREAM_INFO_GROUPS_BATCHED = 6
OEM_CELLS_STREAM_INFO_ARENA_BYTES = 7
OEM_CELLS_STREAM_INFO_BARCODE_MISSES = 8
OEM_CELLS_STREAM_INFO_BARCODE_TABLE_SLOTS = 9
OEM_CELLS_STREAM_INFO_UMI_DUP_READS = 10
OEM_CELLS_STREAM_INFO_UMI_DUP_RECORDS = 11
OEM_CELLS_STREAM_INFO_UMI_CORRECTED_READS = 12
OEM_CELLS_STREAM_INFO_BARCODE_REJECTED = 13
OEM_CELLS_STREAM_INFO_BARCODE_DEFERRED = 14
OEM_RECORDS_STREAM_INFO_BATCHES = 1
OEM_RECORDS_STREAM_INFO_GROUPS = 2
OEM_RECORDS_STREAM_INFO_RECORDS = 3
OEM_RECORDS_STREAM_INFO_BATCHES_BEFORE_FINISH = 4
OEM_RECORDS_STREAM_INFO_BLOCKED_US = 5
OEM_RECORDS_STREAM_INFO_HOST_BATCHES = 6
OEM_RECORDS_STREAM_INFO_ROW_NAME_BYTES = 7
OEM_RECORDS_STREAM_INFO_HOST_FINISHED = 8
OEM_RECORDS_STREAM_INFO_ARENA_BYTES = 9
OEM_INFO_WEIGHT_DICT_ENTRIES = 1
OEM_INFO_TILES = 2
OEM_INFO_REMOTE_ALIGNMENTS = 3
OEM_INFO_RUN_HISTORY_STORED = 4
OEM_TEXT_INFO_CONTENT_BYTES = 1
OEM_TEXT_INFO_BLOCKS = 2
OEM_TEXT_INFO_RAW_BLOCKS = 3
OEM_BARCODE_EXACT, OEM_BARCODE_CORRECTED, OEM_BARCODE_NO_NEIGHBOUR, OEM_BARCODE_AMBIGUOUS, OEM_BARCODE_MISSING = range(5)
OEM_BARCODE_NO_ID = 0xFFFFFFFF
OEM_COLLATE_SORT = 0
OEM_COLLATE_ADJACENT = 1

# every symbol include/oarfish_em.h declares (tests check the .so exports all of them)
ABI_SYMBOLS = [
    "oem_abi_version", "oem_last_error", "oem_device_count",
    "oem_store_create", "oem_store_destroy", "oem_store_dims", "oem_store_bytes", "oem_store_info", "oem_store_set_option",
    "oem_builder_create", "oem_builder_destroy", "oem_builder_add_group", "oem_builder_add_groups",
    "oem_builder_add_groups_device", "oem_store_create_records", "oem_store_create_records_names", "oem_builder_add_projected_group",
    "oem_builder_add_projected_groups", "oem_builder_add_projected_groups_device", "oem_store_create_projected_records",
    "oem_builder_dims",
    "oem_builder_discard_table", "oem_builder_export", "oem_builder_coverage_probs",
    "oem_builder_coverage_probs_binomial", "oem_coverage_probs_device", "oem_builder_coverage_probs_device",
    "oem_coverage_probs_cells_device",
    "oem_builder_store_create", "oem_store_create_coverage", "oem_builder_store_create_coverage",
    "oem_m_step", "oem_em_run", "oem_run_history", "oem_aux_counts", "oem_assignment_probs",
    "oem_assignment_text", "oem_text_result_dims", "oem_text_result_copy", "oem_text_result_destroy",
    "oem_assignment_text_lz4", "oem_text_result_info", "oem_count_matrix_text", "oem_cells_gene_counts",
    "oem_quant_text", "oem_ambig_text",
    "oem_bootstrap_weights", "oem_bootstrap",
    "oem_em_run_cells", "oem_em_run_cells_sparse", "oem_cells_result_dims", "oem_cells_result_copy",
    "oem_cells_result_destroy", "oem_em_run_cells_coverage_sparse",
    "oem_em_run_cells_records_sparse", "oem_cells_result_discard_tables", "oem_collate_names",
    "oem_em_run_cells_records_names_sparse", "oem_collate_barcodes", "oem_em_run_cells_records_barcodes_sparse",
    "oem_dedup_umis", "oem_em_run_cells_records_umis_sparse",
    "oem_dedup_umis_rule", "oem_em_run_cells_records_umis_rule_sparse",
    "oem_correct_barcodes", "oem_em_run_cells_records_whitelist_sparse",
    "oem_cells_stream_create", "oem_cells_stream_push", "oem_cells_stream_set_filters", "oem_cells_stream_push_records",
    "oem_cells_stream_set_barcodes", "oem_cells_stream_push_barcodes", "oem_cells_stream_barcodes_dims",
    "oem_cells_stream_barcodes_copy", "oem_cells_stream_set_barcodes_any_order",
    "oem_cells_stream_set_umis", "oem_cells_stream_push_barcodes_umis", "oem_cells_stream_umis_copy",
    "oem_cells_stream_set_umi_rule", "oem_cells_stream_umi_rule_copy",
    "oem_cells_stream_set_whitelist", "oem_cells_stream_whitelist_copy",
    "oem_cells_stream_finish", "oem_cells_stream_info", "oem_cells_stream_destroy",
    "oem_records_stream_create", "oem_records_stream_push", "oem_records_stream_finish", "oem_records_stream_info",
    "oem_records_stream_destroy", "oem_records_stream_set_names", "oem_records_stream_push_names",
    "oem_records_stream_finish_names", "oem_records_stream_names_copy", "oem_records_stream_set_projected",
    "oem_records_stream_push_projected", "oem_records_stream_set_sort", "oem_records_stream_push_sort",
    "oem_records_stream_order_copy",
    "oem_comm_unique_id", "oem_comm_create", "oem_comm_destroy", "oem_comm_p2p_export", "oem_comm_p2p_connect",
    "oem_comm_set_option", "oem_comm_info", "oem_store_attach_comm",
    "oem_time_m_step", "oem_time_em_iters", "oem_time_bootstrap_passes", "oem_time_allreduce",
    "oem_cells_last_timing",
]


class OemError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"oarfish_em error {code}: {msg}")
        self.code = code


class RunInfoC(C.Structure):
    _fields_ = [
        ("niter", C.c_uint32),
        ("n_passes", C.c_uint32),
        ("converged", C.c_uint32),
        ("reserved", C.c_uint32),
        ("rel_diff", C.c_double),
    ]


class FiltersC(C.Structure):
    _fields_ = [("five_prime_clip", C.c_uint32), ("three_prime_clip", C.c_int64),
                ("score_threshold", C.c_float), ("min_aligned_fraction", C.c_float),
                ("min_aligned_len", C.c_uint32), ("which_strand", C.c_int32),
                ("score_prob_denom", C.c_float), ("reserved", C.c_uint32)]


class AlnRecordC(C.Structure):
    _fields_ = [("ref_id", C.c_uint32), ("aln_start", C.c_uint32), ("aln_end", C.c_uint32),
                ("aln_span", C.c_uint32), ("score", C.c_int64), ("seq_len", C.c_int64),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class DiscardTableC(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("discard_5p", "discard_3p", "discard_score", "discard_aln_frac",
                                          "discard_aln_len", "discard_ori", "discard_supp", "valid_best_aln",
                                          "no_mapping", "no_valid_aln")]


REC_UNMAPPED, REC_REVERSE, REC_SUPPLEMENTARY, REC_HAS_SCORE = 1, 2, 4, 8


class ProjRecordC(C.Structure):
    _fields_ = [("similarity", C.c_double), ("ref_id", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32),
                ("aligned_len", C.c_uint32), ("query_aligned_len", C.c_uint32), ("aln_score", C.c_int32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class ProjOptsC(C.Structure):
    _fields_ = [("beta", C.c_float), ("prob_source", C.c_int32)]


PROJ_SIMILARITY, PROJ_SCORE, PROJ_COMBINED = 0, 1, 2


class CellsStreamOptsC(C.Structure):
    _fields_ = [("n_txps", C.c_uint32), ("device", C.c_int32), ("max_iter", C.c_uint32), ("conv_thresh", C.c_double),
                ("coverage", C.c_uint32), ("bin_width", C.c_uint32), ("model", C.c_int32), ("growth_rate", C.c_double),
                ("group_nnz", C.c_uint64), ("group_cells", C.c_uint32), ("max_staged_nnz", C.c_uint64),
                ("reserved", C.c_uint32 * 4)]


class RecordsStreamOptsC(C.Structure):
    _fields_ = [("n_txps", C.c_uint32), ("device", C.c_int32), ("bin_width", C.c_uint32), ("model", C.c_int32),
                ("growth_rate", C.c_double), ("max_staged_records", C.c_uint64), ("reserved", C.c_uint32 * 4)]


class ParseInfoC(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_unmapped", "n_parsed", "n_groups", "n_reads", "unique_alignments", "n_checked")] \
        + [("reserved", C.c_uint64 * 2)]


class StoreOptsC(C.Structure):
    _fields_ = [("reorder_rows", C.c_uint32), ("problem_size", C.c_uint32), ("window_cap", C.c_uint32),
                ("layout_build", C.c_uint32), ("weight_coding", C.c_uint32), ("reserved", C.c_uint32 * 3)]


_lib = None       # the library the package calls into (the product, unless inside `testing()`)
_product = None
_testing = None
TESTING_LIB_PATH = os.path.join(HERE, "liboarfish_em_testing.so")


def _load(path: str) -> C.CDLL:
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python -m oarfish_amd.build` "
            "(or __graft_entry__.build()).  oarfish_amd has no CPU fallback."
        )
    try:  # make sure the process has ONE HIP runtime / RCCL: torch's, if torch is around
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for the C ABI
        pass
    L = C.CDLL(path)
    vp, u64, u32, i32, f64 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_double
    L.oem_abi_version.restype = i32
    L.oem_last_error.restype = C.c_char_p
    L.oem_device_count.argtypes = [C.POINTER(i32)]
    L.oem_store_create.argtypes = [vp, vp, vp, vp, u64, u64, u32, i32, vp, C.POINTER(vp)]
    L.oem_store_destroy.argtypes = [vp]
    L.oem_store_destroy.restype = None
    L.oem_store_dims.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u32)]
    L.oem_store_bytes.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.oem_store_info.argtypes = [vp, u32, C.POINTER(u64)]
    L.oem_store_set_option.argtypes = [vp, u32, u64]
    L.oem_builder_create.argtypes = [vp, vp, u32, C.POINTER(vp)]
    L.oem_builder_destroy.argtypes = [vp]
    L.oem_builder_destroy.restype = None
    L.oem_builder_add_group.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.oem_builder_add_groups.argtypes = [vp, vp, vp, u64, vp]
    L.oem_builder_add_groups_device.argtypes = [vp, vp, vp, u64, i32, vp]
    L.oem_store_create_records.argtypes = [vp, vp, u32, vp, vp, u64, u32, i32, f64, i32, vp, vp, vp, C.POINTER(vp)]
    L.oem_builder_add_projected_group.argtypes = [vp, vp, u32, u64, vp, C.POINTER(u32)]
    L.oem_builder_add_projected_groups.argtypes = [vp, vp, vp, vp, u64, vp, vp]
    L.oem_builder_add_projected_groups_device.argtypes = [vp, vp, vp, vp, u64, vp, i32, vp]
    L.oem_store_create_projected_records.argtypes = [vp, vp, u32, vp, vp, vp, u64, vp, u32, i32, f64, i32, vp, vp, vp,
                                                     C.POINTER(vp)]
    L.oem_builder_dims.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.oem_builder_discard_table.argtypes = [vp, vp]
    L.oem_builder_export.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.oem_builder_coverage_probs.argtypes = [vp, u32, f64, vp]
    L.oem_builder_coverage_probs_binomial.argtypes = [vp, u32, vp]
    L.oem_coverage_probs_device.argtypes = [vp, vp, vp, vp, vp, u64, u64, u32, u32, i32, f64, i32, vp]
    L.oem_builder_coverage_probs_device.argtypes = [vp, u32, i32, f64, i32, vp]
    L.oem_coverage_probs_cells_device.argtypes = [vp, u32, vp, vp, vp, vp, vp, u64, u64, u32, u32, i32, f64, i32, vp]
    L.oem_builder_store_create.argtypes = [vp, vp, i32, vp, C.POINTER(vp)]
    L.oem_store_create_coverage.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, u32, u32, i32, f64, i32, vp, vp,
                                            C.POINTER(vp)]
    L.oem_builder_store_create_coverage.argtypes = [vp, u32, i32, f64, i32, vp, vp, C.POINTER(vp)]
    L.oem_m_step.argtypes = [vp, vp, vp, vp]
    L.oem_em_run.argtypes = [vp, vp, u32, f64, u32, vp, C.POINTER(RunInfoC)]
    L.oem_run_history.argtypes = [vp, u32, vp, u32, C.POINTER(u32)]
    L.oem_aux_counts.argtypes = [vp, vp, vp]
    L.oem_assignment_probs.argtypes = [vp, vp, f64, vp]
    L.oem_assignment_text.argtypes = [vp, vp, f64, vp, vp, C.POINTER(vp)]
    L.oem_text_result_dims.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.oem_text_result_copy.argtypes = [vp, vp, vp, vp]
    L.oem_text_result_destroy.argtypes = [vp]
    L.oem_text_result_destroy.restype = None
    L.oem_assignment_text_lz4.argtypes = [vp, vp, f64, vp, vp, vp, u64, C.POINTER(vp)]
    L.oem_text_result_info.argtypes = [vp, u32, C.POINTER(u64)]
    L.oem_count_matrix_text.argtypes = [vp, u32, vp, vp, u32, u32, vp, u64, i32, C.POINTER(vp)]
    L.oem_cells_gene_counts.argtypes = [vp, u32, vp, vp, vp, u32, u32, i32, C.POINTER(vp)]
    L.oem_quant_text.argtypes = [vp, vp, vp, vp, u32, vp, u64, i32, C.POINTER(vp)]
    L.oem_ambig_text.argtypes = [vp, vp, u32, vp, u64, i32, C.POINTER(vp)]
    L.oem_bootstrap_weights.argtypes = [vp, u64, u32, vp]
    L.oem_bootstrap.argtypes = [vp, u32, u64, vp, vp, u32, f64, vp, vp]
    L.oem_em_run_cells.argtypes = [vp, u32, vp, vp, vp, vp, u64, u64, u32, i32, u32, f64, vp, vp]
    L.oem_em_run_cells_sparse.argtypes = [vp, u32, vp, vp, vp, vp, u64, u64, u32, i32, u32, f64, C.POINTER(vp)]
    L.oem_cells_result_dims.argtypes = [vp, C.POINTER(u32), C.POINTER(u64)]
    L.oem_cells_result_copy.argtypes = [vp, vp, vp, vp, vp]
    L.oem_cells_result_destroy.argtypes = [vp]
    L.oem_cells_result_destroy.restype = None
    L.oem_em_run_cells_coverage_sparse.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, u64, u64, u32, u32, i32, f64, i32,
                                                   u32, f64, vp, C.POINTER(vp)]
    L.oem_em_run_cells_records_sparse.argtypes = [vp, vp, u32, vp, vp, u64, vp, u32, u32, i32, f64, i32, u32, f64, vp,
                                                  C.POINTER(vp)]
    L.oem_cells_result_discard_tables.argtypes = [vp, vp]
    L.oem_collate_names.argtypes = [vp, vp, vp, u64, vp, u32, u32, i32, vp, vp, C.POINTER(u64), vp]
    L.oem_em_run_cells_records_names_sparse.argtypes = [vp, vp, u32, vp, u64, vp, vp, vp, vp, u32, u32, u32, i32, f64, i32,
                                                        u32, f64, vp, vp, C.POINTER(u64), vp, vp, C.POINTER(vp)]
    L.oem_collate_barcodes.argtypes = [vp, vp, u64, i32, vp, vp, C.POINTER(u64)]
    L.oem_em_run_cells_records_barcodes_sparse.argtypes = [vp, vp, u32, vp, u64, vp, vp, vp, vp, vp, u32, u32, i32, f64, i32,
                                                           u32, f64, vp, vp, C.POINTER(u64), vp, C.POINTER(u64), vp, vp,
                                                           C.POINTER(vp)]
    L.oem_dedup_umis.argtypes = [vp, vp, vp, u64, vp, u64, vp, u64, vp, u32, i32, vp, vp, vp]
    L.oem_em_run_cells_records_umis_sparse.argtypes = [vp, vp, u32, vp, u64, vp, vp, vp, vp, vp, vp, vp, u32, u32, i32, f64, i32,
                                                       u32, f64, vp, C.POINTER(u64), vp, C.POINTER(u64), vp, C.POINTER(u64), vp, vp,
                                                       vp, C.POINTER(vp)]
    L.oem_dedup_umis_rule.argtypes = [vp, vp, vp, vp, vp, u64, vp, u64, vp, u64, vp, u32, i32, vp, vp, vp, vp]
    L.oem_em_run_cells_records_umis_rule_sparse.argtypes = [vp] + L.oem_em_run_cells_records_umis_sparse.argtypes[:-1] + [vp, C.POINTER(vp)]
    L.oem_correct_barcodes.argtypes = [vp, vp, vp, u64, i32, vp, vp, vp, vp, C.POINTER(u64), C.POINTER(u64), vp]
    L.oem_em_run_cells_records_whitelist_sparse.argtypes = [vp] + L.oem_em_run_cells_records_umis_rule_sparse.argtypes[:-1] + [vp, vp, vp, C.POINTER(vp)]
    L.oem_store_create_records_names.argtypes = [vp, vp, u32, vp, u64, vp, vp, vp, u32, u64, u32, i32, f64, i32, vp, vp, vp, vp, vp,
                                                 vp, vp, vp, C.POINTER(vp)]
    L.oem_cells_stream_set_filters.argtypes = [vp, vp, vp]
    L.oem_cells_stream_push_records.argtypes = [vp, vp, vp, u64, C.POINTER(u64)]
    L.oem_cells_stream_set_barcodes.argtypes = [vp, u32]
    L.oem_cells_stream_set_barcodes_any_order.argtypes = [vp, u32]
    L.oem_cells_stream_push_barcodes.argtypes = [vp, vp, u64, vp, vp, vp, vp, vp, C.POINTER(u64)]
    L.oem_cells_stream_barcodes_dims.argtypes = [vp] + [C.POINTER(u64)] * 5
    L.oem_cells_stream_barcodes_copy.argtypes = [vp] * 8
    L.oem_cells_stream_set_umis.argtypes = [vp]
    L.oem_cells_stream_push_barcodes_umis.argtypes = [vp, vp, u64, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64)]
    L.oem_cells_stream_umis_copy.argtypes = [vp, vp]
    L.oem_cells_stream_set_umi_rule.argtypes = [vp, vp]
    L.oem_cells_stream_umi_rule_copy.argtypes = [vp, vp]
    L.oem_cells_stream_set_whitelist.argtypes = [vp, vp]
    L.oem_cells_stream_whitelist_copy.argtypes = [vp, vp, vp, vp]
    L.oem_cells_stream_create.argtypes = [C.POINTER(CellsStreamOptsC), vp, C.POINTER(vp)]
    L.oem_cells_stream_push.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, C.POINTER(u64)]
    L.oem_cells_stream_finish.argtypes = [vp, C.POINTER(vp)]
    L.oem_cells_stream_info.argtypes = [vp, u32, C.POINTER(u64)]
    L.oem_cells_stream_destroy.argtypes = [vp]
    L.oem_cells_stream_destroy.restype = None
    L.oem_records_stream_create.argtypes = [C.POINTER(RecordsStreamOptsC), vp, vp, C.POINTER(vp)]
    L.oem_records_stream_push.argtypes = [vp, vp, vp, u64, C.POINTER(u64)]
    L.oem_records_stream_finish.argtypes = [vp, vp, vp, vp, C.POINTER(vp)]
    L.oem_records_stream_info.argtypes = [vp, u32, C.POINTER(u64)]
    L.oem_records_stream_destroy.argtypes = [vp]
    L.oem_records_stream_destroy.restype = None
    L.oem_records_stream_set_names.argtypes = [vp, u64]
    L.oem_records_stream_push_names.argtypes = [vp, vp, u64, vp, vp, C.POINTER(u64)]
    L.oem_records_stream_finish_names.argtypes = [vp, vp, vp, vp, C.POINTER(vp)]
    L.oem_records_stream_names_copy.argtypes = [vp, vp, vp, vp, vp]
    L.oem_records_stream_set_projected.argtypes = [vp, vp]
    L.oem_records_stream_push_projected.argtypes = [vp, vp, vp, vp, u64, C.POINTER(u64)]
    L.oem_records_stream_set_sort.argtypes = [vp]
    L.oem_records_stream_push_sort.argtypes = [vp, vp, u64, vp, vp, vp, C.POINTER(u64)]
    L.oem_records_stream_order_copy.argtypes = [vp, vp]
    L.oem_comm_unique_id.argtypes = [vp]
    L.oem_comm_create.argtypes = [vp, i32, i32, i32, C.POINTER(vp)]
    L.oem_comm_destroy.argtypes = [vp]
    L.oem_comm_destroy.restype = None
    L.oem_comm_p2p_export.argtypes = [vp, u64, vp]
    L.oem_comm_p2p_connect.argtypes = [vp, vp]
    L.oem_comm_set_option.argtypes = [vp, u32, u64]
    L.oem_comm_info.argtypes = [vp, u32, C.POINTER(u64)]
    L.oem_time_allreduce.argtypes = [vp, u32, C.POINTER(C.c_float)]
    L.oem_store_attach_comm.argtypes = [vp, vp, u64, u64]
    L.oem_time_m_step.argtypes = [vp, u32, C.POINTER(C.c_float)]
    L.oem_time_em_iters.argtypes = [vp, u32, C.POINTER(C.c_float)]
    L.oem_time_bootstrap_passes.argtypes = [vp, u32, C.POINTER(C.c_float), C.POINTER(u32), C.POINTER(u64)]
    L.oem_cells_last_timing.argtypes = [C.POINTER(C.c_float), C.POINTER(u64)]
    for name in ABI_SYMBOLS:
        getattr(L, name)
    return L


def lib() -> C.CDLL:
    """The library in use: the product (liboarfish_em.so), loaded once; raises if it has not been
    built.  Inside `with testing():` it is the test-only build instead."""
    global _lib, _product
    if _lib is None:
        if _product is None:
            _product = _load(LIB_PATH)
        _lib = _product
    return _lib


def testing_lib() -> C.CDLL:
    """liboarfish_em_testing.so: the product objects plus the hooks of csrc/oem_testing.hip and the
    environment-driven knobs (-DOEM_TESTING).  Only tests/ and scripts/ load it."""
    global _testing
    if _testing is None:
        L = _load(TESTING_LIB_PATH)
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.oem_debug_layout_hash.argtypes = [vp, vp, u32]
        L.oem_debug_local_comm_create.argtypes = [i32, i32, vp]
        L.oem_test_reldiff_stress.argtypes = [u32, u32, u32, i32, vp]
        L.oem_debug_cells_last_paths.argtypes = [vp, vp, u32]
        L.oem_debug_last_launch.argtypes = [vp, vp, u32]
        L.oem_debug_text_last_timing.argtypes = [vp]
        L.oem_debug_text_lz4_last_timing.argtypes = [vp]
        L.oem_test_lz4_frame.argtypes = [vp, u64, vp, u64, C.POINTER(u64)]
        L.oem_debug_filter_last_timing.argtypes = [vp]
        L.oem_debug_mtx_last_timing.argtypes = [vp]
        L.oem_debug_proj_last_pass.argtypes = [vp]
        L.oem_debug_quant_last_call.argtypes = [vp]
        L.oem_debug_collate_last_call.argtypes = [vp]
        L.oem_test_collate_host.argtypes = [vp, vp, vp, u64, vp, u32, u32, u32, vp, vp, C.POINTER(u64), vp]
        L.oem_debug_collate_barcodes_last_call.argtypes = [vp]
        L.oem_debug_cells_barcodes_last_call.argtypes = [vp]
        L.oem_debug_barcode_table_last.argtypes = [vp]
        L.oem_test_collate_barcodes_host.argtypes = [vp, vp, u64, vp, vp, C.POINTER(u64)]
        L.oem_test_dedup_umis_host.argtypes = [vp, vp, vp, u64, vp, u64, vp, u64, vp, u32, vp, vp, vp]
        L.oem_test_dedup_umis_rule_host.argtypes = [vp, vp, vp, vp, vp, u64, vp, u64, vp, u64, vp, u32, vp, vp, vp, vp]
        L.oem_debug_dedup_rule_last_call.argtypes = [vp]
        L.oem_test_correct_barcodes_host.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, C.POINTER(u64), C.POINTER(u64), vp]
        L.oem_test_correct_barcodes_stream_host.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64), C.POINTER(u64), vp, vp]
        L.oem_test_cells_gene_counts_host.argtypes = [vp, u32, vp, vp, vp, u32, u32, C.POINTER(vp)]
        L.oem_debug_gene_counts_last_call.argtypes = [vp]
        L.oem_test_shortest_f64.argtypes = [vp, u64, vp, u64, vp]
        L.oem_debug_cells_records_last_csr.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.oem_debug_records_stream_finish_csr.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.oem_debug_records_stream_last_join.argtypes = [vp]
        L.oem_debug_records_names_last_call.argtypes = [vp]
        L.oem_test_parse_bulk_host.argtypes = [vp, u64, vp, vp, vp, u32, u64, vp, vp, vp]
        L.oem_test_lane_runs.argtypes = [u32, vp, vp, u32, u32, vp, vp, i32]
        L.oem_test_remote_fold.argtypes = [vp, u32, vp, vp, vp, u32, u32, u32, u32, i32, i32]
        L.oem_test_remote_fold_b.argtypes = [vp, u32, vp, vp, vp, vp, u32, u32, vp, u32, i32]
        L.oem_test_multi_fold_reldiff.argtypes = [vp, u32, vp, vp, vp, vp, vp, u32, u32, vp, vp, i32]
        _testing = L
    return _testing


class testing:
    """Context manager: every call of the package goes to the test-only library inside the block
    (handles created inside must be closed inside: the two libraries do not share state)."""

    def __enter__(self):
        global _lib
        lib()
        self._prev = _lib
        _lib = testing_lib()
        return _lib

    def __exit__(self, *exc):
        global _lib
        _lib = self._prev


def check(rc: int) -> None:
    if rc != OEM_OK:
        msg = lib().oem_last_error()
        raise OemError(rc, msg.decode("utf-8", "replace") if msg else "")


def device_count() -> int:
    n = C.c_int(0)
    check(lib().oem_device_count(C.byref(n)))
    return int(n.value)
