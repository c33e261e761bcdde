/*
 * oarfish_em.h -- C ABI of the MI355X-native EM quantification engine.
 *
 * This is the drop-in boundary for oarfish's abundance-estimation hot path
 * (COMBINE-lab/oarfish v0.10.3, src/em.rs + src/bootstrap.rs).  The reference
 * has no FFI layer; the seam it would bind is three Rust functions
 *     em::em      (src/em.rs:262)   -> oem_em_run(..., min_iter_gate = 50)
 *     em::em_par  (src/em.rs:320)   -> oem_em_run(..., min_iter_gate = 1)
 *     em::bootstrap (src/em.rs:292) -> oem_bootstrap
 * over an `EMInfo` (src/util/oarfish_types.rs:408-428), whose `eq_map`
 * (`InMemoryAlignmentStore`, :548-558) becomes an `oem_store` handle that keeps
 * the sparse read x transcript conditional-probability matrix resident in HBM.
 * INTEGRATION.md shows the Rust `extern "C"` block + shim a maintainer adds.
 *
 * Conventions
 *   - plain pointers and sizes only; all host buffers are caller-owned and are
 *     never retained after the call returns (the store is copied to HBM);
 *   - every entry point returns an `oem_status` (0 = OK) and never aborts or
 *     throws across the boundary (the reference's EM is infallible and built
 *     with panic=abort, Cargo.toml:118; a GPU library cannot be);
 *   - `oem_last_error()` gives the thread-local message of the last failure;
 *   - calls on distinct handles are thread-safe (single_cell.rs:96-150 calls
 *     em::em concurrently from N workers); calls on one handle are serialised.
 *   - there is NO CPU fallback: without a HIP device every compute entry point
 *     fails with OEM_ERR_NO_DEVICE.
 */
#ifndef OARFISH_EM_H
#define OARFISH_EM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: oem_time_bootstrap_passes, oem_store_opts.layout_build and .weight_coding (were reserved words: zero = the
 *    default, as before), the peer-to-peer communicator entry points (oem_comm_p2p_*), oem_store_info; version 1
 *    callers keep working (additions only).  Later additions under the same number: the sparse per-cell results
 *    (oem_em_run_cells_sparse, oem_cells_result_dims / _copy / _destroy), the per-cell coverage model
 *    (oem_coverage_probs_cells_device), both in one call (oem_em_run_cells_coverage_sparse), the bulk coverage model
 *    and the store on its column in one call (oem_store_create_coverage, oem_builder_store_create_coverage), the
 *    per-cell session (oem_cells_stream_*), the per-iteration rel_diff record (OEM_OPT_RUN_HISTORY, oem_run_history),
 *    the `.prob` body as text formatted on the device (oem_assignment_text, oem_text_result_dims / _copy / _destroy),
 *    the whole `.prob.lz4` file as one LZ4 frame compressed on the device (oem_assignment_text_lz4,
 *    oem_text_result_info), the batched filter on the host and on the device and the store straight from the records
 *    (oem_builder_add_groups, oem_builder_add_groups_device, oem_store_create_records), the `.count.mtx` file of the
 *    single-cell path as text formatted on the device (oem_count_matrix_text), the projected filter of genome mode
 *    (oem_proj_record, oem_proj_opts, oem_builder_add_projected_group / _groups / _groups_device,
 *    oem_store_create_projected_records), the `.quant` and `.ambig_info.tsv` files of the bulk path as text formatted on
 *    the device (oem_quant_text, oem_ambig_text), a cell's records collated by read name on the device
 *    (oem_collate_names), the bulk records session (oem_records_stream_*), the collation and the records call in one
 *    (oem_em_run_cells_records_names_sparse), cells found from barcodes in any record order (oem_collate_barcodes,
 *    oem_em_run_cells_records_barcodes_sparse). */
#define OEM_ABI_VERSION 2

typedef enum {
    OEM_OK = 0,
    OEM_ERR_ARG = 1,       /* NULL / inconsistent argument (bad row_ptr, tid >= n_txps ...) */
    OEM_ERR_OOM = 2,       /* host or device allocation failed */
    OEM_ERR_HIP = 3,       /* HIP runtime error */
    OEM_ERR_RCCL = 4,      /* RCCL error / librccl not loadable */
    OEM_ERR_NO_DEVICE = 5, /* no usable HIP device */
    OEM_ERR_STATE = 6      /* handle used in a state that does not allow the call */
} oem_status;

/* src/util/constants.rs:1-2 */
#define OEM_MIN_READ_THRESH 1e-5
#define OEM_EM_DENOM_THRESH 1e-30

/* Opaque handles. */
typedef struct oem_store oem_store; /* InMemoryAlignmentStore resident on one GPU (one row shard) */
typedef struct oem_comm oem_comm;   /* RCCL communicator over the row shards of one node */
typedef struct oem_cells_result oem_cells_result; /* sparse per-cell results, host-resident, immutable once returned */
typedef struct oem_text_result oem_text_result;   /* host-resident, immutable once returned */

/* What do_em / em_par leave behind besides the counts. */
typedef struct {
    uint32_t niter;     /* value of `niter` at loop exit (em.rs:170,218 / :354,405) */
    uint32_t n_passes;  /* E/M passes executed, including the final one (em.rs:245 / :433) */
    uint32_t converged; /* 1 if the loop left through `break` (em.rs:212-214 / :399-401) */
    uint32_t reserved;
    double rel_diff;    /* rel_diff of the last loop pass (em.rs:194-201), as logged at :219-233 */
} oem_run_info;

/* Layout / tuning knobs of a store (all optional; zero = default). */
typedef struct {
    uint32_t reorder_rows; /* 0 = default (locality reorder on), 1 = keep caller order, 2 = force reorder */
    uint32_t problem_size; /* 0 = one EM problem; > 0: the transcript space is the concatenation of
                              independent problems of this many transcripts (tiles never mix them);
                              set by oem_em_run_cells for its per-cell batches */
    uint32_t window_cap;   /* transcripts per tile window: 0 = chosen from the store (large and sparse -- at least
                              1 M reads, fewer than 2 per transcript: 2048; else 512), or 512 / 2048 to force it */
    uint32_t layout_build; /* 0 = build the tiled layout on the device (the host builder takes the stores the
                              device builder declines); 1 = always the host builder (oem_layout.cpp, the
                              specification the device builder is tested against) */
    uint32_t weight_coding; /* 0 = a store with at most 1024 distinct f32 weights (as_prob is exp of an integer score
                              gap over a constant: tens to hundreds of values) keeps its weights as indices into a
                              table of them -- in the spare bits of the window codes up to 128 values, a byte each up
                              to 256, 16 bits each up to 1024 (wide-window stores: up to 256, a byte each); lossless,
                              oem_layout_dict.hip; 1 = always the f32 stream (was reserved[0]); 2 = opt-in for stores
                              with a coverage column: the static weight (p as f64) * cov (em.rs:107-111) is rounded
                              once to f32 (relative error <= 6e-8 per weight, against the 1e-4 the abundances are held
                              to) and the store streams 8 B per alignment through the f32 kernels instead of 12 through
                              the f64 ones; all arithmetic of the EM stays f64.  Without cov_prob: the same as 0.
                              Underflow: a product below 1.2e-38 (FLT_MIN) is stored as an f32 subnormal, with fewer
                              significant bits; one below 1.4e-45 (FLT_TRUE_MIN, half of it rounding to nearest) becomes
                              0, so a read whose products all do has denominator 0 and is dropped by the EM's
                              `denom > 1e-30` test (em.rs:115) where the f64 store would keep it */
    uint32_t reserved[3];
} oem_store_opts;

/* --------------------------------------------------------------------- */
/* library                                                                */
/* --------------------------------------------------------------------- */
int oem_abi_version(void);
const char *oem_last_error(void);
int oem_device_count(int *out_count);

/* --------------------------------------------------------------------- */
/* alignment store                                                        */
/* --------------------------------------------------------------------- */

/* Replaces InMemoryAlignmentStore as em.rs reads it (oarfish_types.rs:548-558
 * via iter(), :651-656): row_ptr == boundaries (n_reads+1 entries, row_ptr[0]==0,
 * strictly increasing: the reference never stores an empty read, :724,735-737;
 * empty rows are tolerated and contribute nothing), tid == alignments[].ref_id,
 * as_prob == as_probabilities (f32, :552), cov_prob == coverage_probabilities
 * (f64) or NULL when filter_opts.model_coverage is false (em.rs:108).
 * `device` is the HIP device ordinal.  The arrays are copied to HBM, laid out
 * for the E/M kernels, and may be freed by the caller on return. */
int oem_store_create(const uint64_t *row_ptr, const uint32_t *tid, const float *as_prob,
                     const double *cov_prob, uint64_t n_reads, uint64_t nnz, uint32_t n_txps,
                     int device, const oem_store_opts *opts, oem_store **out);
void oem_store_destroy(oem_store *store);

/* Tuning switches of a store (not part of the reference's semantics; results are
 * unchanged up to floating-point summation order). */
typedef enum {
    OEM_OPT_BATCH_BOOTSTRAP = 1, /* value 1 (default): oem_bootstrap runs its replicates in batches that share
                                    each pass over the matrix (4 per pass, two such chains side by side on their
                                    own streams) when it can (narrow window cap, multiplicities < 256); 0: one per pass */
    OEM_OPT_BOOTSTRAP_FIRST_REPLICA = 2, /* value b0 (default 0): replicate k of the next oem_bootstrap calls
                                    draws the device resample of global replica b0 + k.  Lets N processes
                                    that each hold the whole store split one set of replicates with no
                                    collective (the reference's replicates are independent, em.rs:303-309).
                                    b0 <= 2^32 - 1, and an oem_bootstrap call that draws its resamples must keep
                                    b0 + n_boot - 1 <= 2^32 - 1: it returns OEM_ERR_ARG instead of wrapping. */
    OEM_OPT_RUN_HISTORY = 3 /* value K (default 0 = off): every oem_em_run and oem_bootstrap on the store records the
                                    rel_diff of each loop pass (em.rs:194-201, the value logged at :219-233 / :405-419),
                                    the first min(K, max_iter) passes of each run; later passes are counted, not
                                    stored.  Read with oem_run_history.  The lane that takes the stopping decision
                                    writes the 8 bytes; K <= 2^32 - 1, and the record takes min(K, max_iter) doubles on
                                    the device and per replicate on the host.  The per-cell calls do not record. */
} oem_option;
int oem_store_set_option(oem_store *store, uint32_t option, uint64_t value);

/* store.len() / num_aligned_reads() (oarfish_types.rs:562-564,746-748),
 * total_len() (:741-743), txp_info.len(). */
int oem_store_dims(const oem_store *store, uint64_t *n_reads, uint64_t *nnz, uint32_t *n_txps);

/* Bytes of HBM the store occupies and the algorithmic bytes of one E/M pass
 * (nnz*(4+4|8) + (R+1)*4 + 2*T*8). */
int oem_store_bytes(const oem_store *store, uint64_t *hbm_bytes, uint64_t *algorithmic_bytes_per_pass);

/* Facts about the resident layout.  OEM_INFO_WEIGHT_DICT_ENTRIES: entries of the weight table when the local
 * weights are dictionary-coded (oem_store_opts.weight_coding), 0 when the store streams f32 / f64 weights;
 * OEM_INFO_TILES, OEM_INFO_REMOTE_ALIGNMENTS: tiles of the layout and alignments outside their tile's window;
 * OEM_INFO_RUN_HISTORY_STORED: entries per run the last oem_em_run / oem_bootstrap could store under OEM_OPT_RUN_HISTORY,
 * min(K, max_iter) of that call (a run holds the smaller of this and its length); 0 when it recorded nothing. */
typedef enum { OEM_INFO_WEIGHT_DICT_ENTRIES = 1, OEM_INFO_TILES = 2, OEM_INFO_REMOTE_ALIGNMENTS = 3,
               OEM_INFO_RUN_HISTORY_STORED = 4 } oem_store_info_key;
int oem_store_info(const oem_store *store, uint32_t key, uint64_t *value);

/* --------------------------------------------------------------------- */
/* store builder: the step right before the EM (host side; only the *_device entry points use the GPU) */
/* --------------------------------------------------------------------- */

/* AlignmentFilters (src/util/oarfish_types.rs:763-806), the fields filter() reads. */
typedef struct {
    uint32_t five_prime_clip;    /* :768 */
    int64_t three_prime_clip;    /* :772 */
    float score_threshold;       /* :778 */
    float min_aligned_fraction;  /* :782 */
    uint32_t min_aligned_len;    /* :786 */
    int32_t which_strand;        /* :789  0 = Unknown (both), 1 = Forward only, 2 = Reverse only */
    float score_prob_denom;      /* :804  D in exp((score - best) / D), default 5.0 */
    uint32_t reserved;
} oem_filters;

/* One alignment record as AlnRecordLike exposes it (src/util/oarfish_types.rs:180-202, :264-326). */
typedef struct {
    uint32_t ref_id;     /* ref_id() */
    uint32_t aln_start;  /* aln_start() */
    uint32_t aln_end;    /* aln_end() */
    uint32_t aln_span;   /* aln_span() */
    int64_t score;       /* aln_score(); ignored unless OEM_REC_HAS_SCORE */
    int64_t seq_len;     /* opt_sequence_len(); < 0 = None */
    uint32_t flags;      /* OEM_REC_* */
    uint32_t reserved;
} oem_aln_record;
#define OEM_REC_UNMAPPED 1u      /* is_unmapped() */
#define OEM_REC_REVERSE 2u       /* is_reverse_complemented() */
#define OEM_REC_SUPPLEMENTARY 4u /* is_supp() */
#define OEM_REC_HAS_SCORE 8u     /* aln_score() is Some */

/* DiscardTable (src/util/oarfish_types.rs:811-857). */
typedef struct {
    uint64_t discard_5p, discard_3p, discard_score, discard_aln_frac, discard_aln_len, discard_ori,
        discard_supp, valid_best_aln, no_mapping, no_valid_aln;
} oem_discard_table;

typedef struct oem_builder oem_builder;

/* InMemoryAlignmentStore::new + the transcript lengths filter() needs (TranscriptInfo.len). */
int oem_builder_create(const oem_filters *filters, const uint64_t *txp_len, uint32_t n_txps,
                       oem_builder **out);
void oem_builder_destroy(oem_builder *b);
/* InMemoryAlignmentStore::add_group (src/util/oarfish_types.rs:672-685): AlignmentFilters::filter
 * (:955-1130: strand / supplementary / length / 3' / 5' filters, best-score tracking, aligned-
 * fraction test, score threshold, as_prob = expf((score - best) / D) in f32, :1107-1113) followed by
 * add_filtered_group (:718-738).  *out_kept = alignments appended (0: the read was dropped).
 * The coverage intervals add_filtered_group also updates (:725-728) are recomputed from the retained
 * alignments by the coverage entry points below. */
int oem_builder_add_group(oem_builder *b, const oem_aln_record *records, uint32_t n_records,
                          uint32_t *out_kept);
/* n_groups add_group calls in one: group g = records[group_off[g] .. group_off[g+1]) (group_off: n_groups + 1 entries).
 * The builder's state afterwards -- everything oem_builder_export, _dims and _discard_table show -- is byte for byte the
 * state after the loop of oem_builder_add_group over the same groups in order; appending to a non-empty builder works.
 * out_kept[g] (n_groups entries, or NULL) is what add_group would have returned for group g; row r of what the call
 * appends is the r-th group with out_kept > 0, which is how a caller lines read names up for oem_assignment_text.
 * The call is atomic: on any error the builder is unchanged.  Argument errors are those of add_group plus those of
 * group_off (NULL, group_off[0] != 0, decreasing, a group of more than 2^32 - 1 records); a ref_id that is not below
 * n_txps is reported with the index of the first such record. */
int oem_builder_add_groups(oem_builder *b, const oem_aln_record *records, const uint64_t *group_off,
                           uint64_t n_groups, uint32_t *out_kept /* n_groups, or NULL */);
/* The same builder state afterwards, byte for byte, computed on the device (oem_filter_device.hip): the records go up
 * in chunks, one lane filters each read, the retained alignments are compacted on the device and copied back.  The f32
 * as_prob is bit-identical to the host's because the device never computes exp: the host fills a table
 * tab[g] = expf((float)(-g) / D) over the integer score gap g = best - score, up to the first entry that is +0.0f, and
 * the device looks as_prob up by g (exact for |score| <= 2^24).  The batch goes through the host loop of
 * oem_builder_add_groups instead -- same result -- when score_prob_denom is not finite and positive, when the table
 * would need more than 2^22 entries, or when a mapped record with OEM_REC_HAS_SCORE has |(int32_t)score| > 2^24 (found
 * by the device pass, which the host then repeats).  The result does not depend on how the call cuts its input into
 * chunks.  At most 2^31 - 2 groups per call (OEM_ERR_ARG).  Without a device: OEM_ERR_NO_DEVICE -- also for a batch
 * the host loop will take (the device is asked for before the fallback is chosen, so the call never succeeds on a box
 * where its device form could not run). */
int oem_builder_add_groups_device(oem_builder *b, const oem_aln_record *records, const uint64_t *group_off,
                                  uint64_t n_groups, int device, uint32_t *out_kept);
int oem_builder_dims(const oem_builder *b, uint64_t *n_reads, uint64_t *nnz);
int oem_builder_discard_table(const oem_builder *b, oem_discard_table *out);
/* Copies the store out: row_ptr[n_reads+1], and per alignment tid / as_prob / start / end / strand
 * (0 forward, 1 reverse); any output pointer may be NULL. */
int oem_builder_export(const oem_builder *b, uint64_t *row_ptr, uint32_t *tid, float *as_prob,
                       uint32_t *start, uint32_t *end, uint8_t *strand);
/* The bulk coverage model: per-transcript binned coverage of the
 * retained alignments (TranscriptInfo::with_len_and_bin_width + add_interval,
 * src/util/oarfish_types.rs:460-468, :496-538), the clamped logistic bin probabilities
 * (logistic_prob, src/util/logistic_probability.rs:7-79; min coverage total_weight/100, f32 bin
 * counts) and the per-alignment coverage probability normalised to sum 1 per read
 * (normalize_read_probs, src/util/normalize_probability.rs:5-74).  out_cov_prob: nnz f64 in the
 * builder's alignment order -- the `cov_prob` column of oem_store_create.  bin_width: --bin-width
 * (prog_opts.rs:555, default 100); growth_rate: --growth-rate (prog_opts.rs:502, default 2.0).
 * Where the reference would panic (degenerate bins, non-finite probability) this returns
 * OEM_ERR_STATE. */
int oem_builder_coverage_probs(const oem_builder *b, uint32_t bin_width, double growth_rate,
                               double *out_cov_prob);
/* The single-cell coverage model: same bins and the same per-read normalisation, but the bin
 * probabilities are binomial_continuous_prob's (src/util/binomial_probability.rs:7-224; called per
 * cell at src/single_cell.rs:132-137): Binomial pmf of each bin's count, counts rescaled so the
 * largest is 709, normalised over the transcript's bins.  ln_gamma is libm's lgamma (the reference
 * uses statrs' Lanczos evaluation of the same function). */
int oem_builder_coverage_probs_binomial(const oem_builder *b, uint32_t bin_width, double *out_cov_prob);
/* Both coverage models on the device (oem_coverage_device.hip): the same f64 arithmetic, one thread per
 * alignment / transcript / read; the bins are summed with f64 atomics, so results agree with the host
 * functions above to the last few bits (and to ~1e-7 where a bin count sits on an f32 rounding boundary,
 * the reference's f32 truncation of the counts, oarfish_types.rs:478).  model: 0 = logistic
 * (growth_rate used), 1 = binomial.  Arrays are the caller's (host) CSR with the alignment coordinates
 * AlnInfo carries (start / end, oarfish_types.rs:330-337); out_cov_prob: nnz f64. */
int oem_coverage_probs_device(const uint64_t *row_ptr, const uint32_t *tid, const uint32_t *aln_start,
                              const uint32_t *aln_end, const uint64_t *txp_len, uint64_t n_reads, uint64_t nnz,
                              uint32_t n_txps, uint32_t bin_width, int model, double growth_rate, int device,
                              double *out_cov_prob);
int oem_builder_coverage_probs_device(const oem_builder *b, uint32_t bin_width, int model, double growth_rate,
                                      int device, double *out_cov_prob);
/* The per-cell coverage model of a single-cell run (single_cell.rs:117-137: every cell bins only its own
 * retained alignments and normalises its own reads), for all cells in one call.  Cells as in oem_em_run_cells:
 * one concatenated CSR plus cell_row_off[n_cells+1]; aln_start / aln_end / out_cov_prob: nnz each, the caller's
 * alignment order.  The result is, cell by cell, what oem_coverage_probs_device returns on that cell's slice (row_ptr
 * rebased to 0), up to the order of the f64 atomic sums.  Bins are allocated only for the (cell, transcript) pairs
 * that occur, in chunks of consecutive cells that fit in device memory.  Cells without reads are allowed; nnz must
 * be below 2^32 and n_txps below 2^31 - 1.  OEM_ERR_STATE conditions are those of oem_coverage_probs_device; the
 * message names the first offending cell. */
int oem_coverage_probs_cells_device(const uint64_t *cell_row_off, uint32_t n_cells, const uint64_t *row_ptr,
                                    const uint32_t *tid, const uint32_t *aln_start, const uint32_t *aln_end,
                                    const uint64_t *txp_len, uint64_t n_reads, uint64_t nnz, uint32_t n_txps,
                                    uint32_t bin_width, int model, double growth_rate, int device,
                                    double *out_cov_prob);
/* Uploads the built store (oem_store_create on the builder's arrays). */
int oem_builder_store_create(const oem_builder *b, const double *cov_prob, int device,
                             const oem_store_opts *opts, oem_store **out);
/* The bulk coverage model (oem_coverage_probs_device) and oem_store_create on its column, in one call: the coordinates
 * go up once, the column and the weights never leave the device.  The store is the one oem_coverage_probs_device
 * followed by oem_store_create(row_ptr, tid, as_prob, that column, n_reads, nnz, n_txps, device, opts) gives, for
 * every opts: its weights are bit-identical (w = (double)p * cov; a read with a NaN coverage gets p * 0 on every
 * alignment; weight_coding 2 rounds each product once to f32, see oem_store_opts).  Errors are those of the two calls;
 * argument errors (nnz must be below 2^32) are reported before any device use, an alignment outside its transcript is
 * OEM_ERR_STATE.  out_cov_prob (nnz, optional): the column as oem_coverage_probs_device returns it, NaN included.
 * *out = NULL on any failure. */
int oem_store_create_coverage(const uint64_t *row_ptr, const uint32_t *tid, const float *as_prob,
                              const uint32_t *aln_start, const uint32_t *aln_end, const uint64_t *txp_len,
                              uint64_t n_reads, uint64_t nnz, uint32_t n_txps,
                              uint32_t bin_width, int model, double growth_rate,
                              int device, const oem_store_opts *opts,
                              double *out_cov_prob /* nnz, or NULL */, oem_store **out);
/* The same on the builder's arrays (oem_builder_export's view; n_txps: the builder's transcripts). */
int oem_builder_store_create_coverage(const oem_builder *b, uint32_t bin_width, int model, double growth_rate,
                                      int device, const oem_store_opts *opts,
                                      double *out_cov_prob /* nnz, or NULL */, oem_store **out);
/* records -> resident store in one call; the CSR never exists on the host.  The store is the one the long way round
 * gives: oem_builder_create(filters, txp_len, n_txps), oem_builder_add_groups, then oem_builder_store_create (model -1:
 * no coverage column) or oem_builder_store_create_coverage (model 0 / 1 with bin_width and growth_rate as there), with
 * the same opts, for every weight_coding and both layout_build values (host arrays come back from the device only for
 * the host layout builder).  out_kept (n_groups, or NULL) and out_discard (or NULL) are add_groups' out_kept and the
 * builder's discard table.  Requires fewer than 2^32 kept alignments (OEM_ERR_ARG otherwise); the other argument errors
 * are those of oem_builder_add_groups_device and oem_store_create_coverage, an alignment outside its transcript under a
 * coverage model is OEM_ERR_STATE.  *out = NULL on any failure. */
int oem_store_create_records(const oem_filters *filters, const uint64_t *txp_len, uint32_t n_txps,
                             const oem_aln_record *records, const uint64_t *group_off, uint64_t n_groups,
                             uint32_t bin_width, int model, double growth_rate,
                             int device, const oem_store_opts *opts,
                             uint32_t *out_kept /* n_groups, or NULL */, oem_discard_table *out_discard /* or NULL */,
                             oem_store **out);

/* One projected (transcriptome-space) alignment of a genome-mode read: ProjectedAlnRecord
 * (src/util/oarfish_types.rs:1142-1164).  40 bytes. */
typedef struct {
    double similarity;          /* :1158  higher is better; the best of a read anchors the probability */
    uint32_t ref_id;            /* :1145 */
    uint32_t start;             /* :1147  1-based */
    uint32_t end;               /* :1149  1-based, inclusive */
    uint32_t aligned_len;       /* :1151  transcript bases spanned */
    uint32_t query_aligned_len; /* :1153  read bases aligned, for the aligned fraction */
    int32_t aln_score;          /* :1163  score of the genomic alignment this was projected from */
    uint32_t flags;             /* OEM_REC_REVERSE (is_reverse, :1155); other bits are ignored */
    uint32_t reserved;
} oem_proj_record;

/* What filter_projected takes besides the filters: --projected-prob-beta and ProjProbSource (src/prog_opts.rs:48-57). */
typedef struct {
    float beta;          /* default 10.0 */
    int32_t prob_source; /* OEM_PROJ_SIMILARITY, _SCORE or _COMBINED */
} oem_proj_opts;
#define OEM_PROJ_SIMILARITY 0 /* exp((float)(sim - best_sim) * beta) */
#define OEM_PROJ_SCORE 1      /* exp((float)(score - best_score) / D) */
#define OEM_PROJ_COMBINED 2   /* exp((float)(score - best_score) / D + beta * (float)(sim - best_sim)) */

/* InMemoryAlignmentStore::add_projected_group (src/util/oarfish_types.rs:695-715): AlignmentFilters::filter_projected
 * (:1179-1297) followed by add_filtered_group, for one genome-mode read.  Of oem_filters it reads which_strand,
 * min_aligned_len, three_prime_clip, five_prime_clip, min_aligned_fraction, score_threshold and score_prob_denom.  The
 * first walk discards by orientation, aligned length, 3' and 5' distance, in that order, and tracks the best similarity
 * (the first maximum; it fixes the aligned fraction query_aligned_len / read_len, 0 for read_len 0) and, independently,
 * the best score.  Nothing retained or a best similarity <= 0 (a NaN never becomes the best): no counter moves, no row.
 * An aligned fraction below min_aligned_fraction: discard_aln_frac.  Otherwise valid_best_aln, and a retained record
 * is kept iff (float)(similarity * (1.0 / best)) >= score_threshold (discard_score otherwise), with its interval clamped
 * into [1, txp_len] and as_prob = expf(f), f as under OEM_PROJ_* in f32 (the score difference wraps as i32), expf the
 * host libm's.  no_mapping, no_valid_aln and discard_supp are never counted here.  A row is appended iff an alignment
 * is kept; *out_kept = alignments appended.  A ref_id that is not below n_txps or a transcript of length 0, on any
 * record of the group, is OEM_ERR_ARG (the reference would panic) and leaves the builder unchanged.  Projected and plain
 * groups may be added to one builder in turn. */
int oem_builder_add_projected_group(oem_builder *b, const oem_proj_record *records, uint32_t n_records,
                                    uint64_t read_len, const oem_proj_opts *popts, uint32_t *out_kept);
/* n_groups add_projected_group calls in one, as oem_builder_add_groups is to oem_builder_add_group: the same builder
 * state afterwards byte for byte, the same out_kept, atomic, the same group_off errors; read_len has n_groups entries.
 * An argument error of a record is reported with the index of the first such record. */
int oem_builder_add_projected_groups(oem_builder *b, const oem_proj_record *records, const uint64_t *group_off,
                                     const uint64_t *read_len, uint64_t n_groups, const oem_proj_opts *popts,
                                     uint32_t *out_kept /* n_groups, or NULL */);
/* The same builder state afterwards, byte for byte, computed on the device (oem_filter_projected_device.hip), as
 * oem_builder_add_groups_device is to oem_builder_add_groups.  OEM_PROJ_SCORE looks as_prob up in the host's table over
 * the integer score gap, with that call's fallbacks to the host loop (score_prob_denom, |aln_score| > 2^24).  For
 * OEM_PROJ_SIMILARITY and _COMBINED the argument f is continuous: the device computes (float)exp((double)f) and keeps it
 * only where that is provably what a libm expf returns -- f finite and <= 0, the result not subnormal, the f64 value
 * at least 1/256 of an f32 ulp away from a rounding tie.  The other alignments (about 0.4 %) come down as (index, f),
 * the host applies its expf and the values go back up before anything reads the weights.  A beta that is not finite
 * sends these two sources through the host loop, as does |aln_score| > 2^24 for every source.  The result does not
 * depend on the chunking; at most 2^31 - 2 groups per call; without a device OEM_ERR_NO_DEVICE, as there. */
int oem_builder_add_projected_groups_device(oem_builder *b, const oem_proj_record *records, const uint64_t *group_off,
                                            const uint64_t *read_len, uint64_t n_groups, const oem_proj_opts *popts,
                                            int device, uint32_t *out_kept);
/* Projected records -> resident store in one call, as oem_store_create_records: the store is the one
 * oem_builder_create, oem_builder_add_projected_groups and oem_builder_store_create (model -1) or
 * oem_builder_store_create_coverage (model 0 / 1) give with the same opts; out_kept, out_discard, the limits and the
 * errors are those of that call and of oem_builder_add_projected_groups_device.  *out = NULL on any failure. */
int oem_store_create_projected_records(const oem_filters *filters, const uint64_t *txp_len, uint32_t n_txps,
                                       const oem_proj_record *records, const uint64_t *group_off,
                                       const uint64_t *read_len, uint64_t n_groups, const oem_proj_opts *popts,
                                       uint32_t bin_width, int model, double growth_rate,
                                       int device, const oem_store_opts *opts,
                                       uint32_t *out_kept /* n_groups, or NULL */,
                                       oem_discard_table *out_discard /* or NULL */, oem_store **out);

/* --------------------------------------------------------------------- */
/* EM                                                                     */
/* --------------------------------------------------------------------- */

/* One E/M pass (em.rs:87-133 m_step): out_counts[t] = sum over reads i of
 * row_w[i] * theta[t]*w_it / sum_j theta[t_j]*w_ij, reads with denominator
 * <= 1e-30 dropped (em.rs:115).  row_w == NULL means all ones.  theta and
 * out_counts are host arrays of n_txps f64.  For step-level parity tests and
 * external loop drivers; the fused drivers below never leave the device. */
int oem_m_step(oem_store *store, const double *theta, const uint32_t *row_w, double *out_counts);

/* The EM driver (em.rs:144-255 do_em / :320-447 em_par).
 *   init_abundances : n_txps f64 or NULL => uniform n_reads/n_txps (em.rs:160-167)
 *   max_iter        : EMInfo.max_iter (prog_opts.rs:532, default 1000)
 *   conv_thresh     : EMInfo.convergence_thresh (prog_opts.rs:536, default 1e-3)
 *   min_iter_gate   : 50 reproduces em::em (em.rs:212), 1 reproduces em::em_par (em.rs:399)
 *   out_counts      : n_txps f64, un-normalised expected read counts (em.rs:254)
 *   info            : optional
 * The stopping iteration is the reference's: the loop state is frozen on the
 * device at the first pass that satisfies the gate. */
int oem_em_run(oem_store *store, const double *init_abundances, uint32_t max_iter,
               double conv_thresh, uint32_t min_iter_gate, double *out_counts,
               oem_run_info *info);

/* The rel_diff trajectory of a run recorded under OEM_OPT_RUN_HISTORY: h[k] is the rel_diff of loop pass k
 * (em.rs:194-201, before :234 resets it), k = `niter` as the stopping rule sees it (before em.rs:218, and on the
 * `break` branch), so the reference's line `iteration N; rel diff R` (em.rs:219-233 / :405-419) is h[N-1].  A run has
 * n = info.niter + info.converged = info.n_passes - 1 entries and h[n-1] is info.rel_diff, bit for bit.
 *   run      : 0 after oem_em_run; the replicate index b (row b of `out` / `infos`) after oem_bootstrap
 *   out      : receives min(capacity, recorded) entries; NULL with capacity 0 queries the length alone
 *   out_len  : optional; the run's n, which may exceed what was recorded (oem_store_info: OEM_INFO_RUN_HISTORY_STORED)
 * OEM_ERR_STATE when the last oem_em_run / oem_bootstrap on the store recorded nothing (the option was off, or there has
 * been no run yet); OEM_ERR_ARG for a run out of range.  The record of a call is valid until the next oem_em_run,
 * oem_bootstrap or change of the option on that store. */
int oem_run_history(const oem_store *store, uint32_t run, double *out, uint32_t capacity, uint32_t *out_len);

/* --------------------------------------------------------------------- */
/* the steps right after the EM, on the same resident store                */
/* --------------------------------------------------------------------- */

/* aux_counts::get_aux_counts (src/util/aux_counts.rs:23-50): per transcript, the number of
 * alignments (total) and the number of single-alignment reads (unique); n_txps u32 each. */
int oem_aux_counts(oem_store *store, uint32_t *out_unique, uint32_t *out_total);

/* The E-step of write_function::write_out_prob (src/util/write_function.rs:283-318): per read,
 * nprob_j = clamp(counts[t_j]*p_j*cov_j / sum_j(...), 0, 1); alignments with nprob >=
 * display_thresh are kept and renormalised by their sum.  out_prob is nnz f64 in the caller's
 * alignment order: the probability the reference prints, or -1 for an alignment it omits. */
int oem_assignment_probs(oem_store *store, const double *counts, double display_thresh,
                         double *out_prob);

/* The body of the `.prob` file (write_function.rs:283-332) for every read of the store, in the caller's read and
 * alignment order, as the bytes the reference writes: the E-step above, then per read the line
 *     name '\t' k '\t' id_1 '\t' .. id_k '\t' p_1 '\t' .. p_k '\n'       (a read that keeps nothing: name "\t0\t\t\n")
 * formatted on the device.  k and the ids are plain decimal; each p is Rust's `{:.d}` with d =
 * prob_display_decimals(display_thresh) (:218-224: ceil(-log10(thresh)) in 3 .. 9; 9 for a threshold that is not
 * positive and finite): the exact binary value correctly rounded, ties to even, as glibc's "%.*f" prints it; 0/0
 * (display_thresh <= 0 and every kept nprob zero) prints as `NaN`.  The file's header lines (the counts and the
 * transcript names) are the caller's.
 * names / name_off: the read names as one byte blob and n_reads + 1 offsets (name r = bytes
 * [name_off[r], name_off[r+1])); trailing NUL bytes of a name are dropped (trim_end_matches('\0'), :294).
 * names == NULL (then name_off == NULL too): every name is empty (the line starts with the tab).  counts: n_txps f64.
 * Argument errors (a NULL store / counts / out, names without name_off or the reverse, name_off[0] != 0, name_off
 * decreasing) are reported before any device use; *out is NULL after any failure.  Like oem_assignment_probs the call
 * overwrites the store's theta scratch (no other state), works on every kind of store (f32 / f64 weights, any
 * weight_coding, wide row pointers, oem_store_create_coverage), and a row shard produces the lines of its own reads.
 * The text leaves the device in chunks of consecutive reads (256 MiB of text each, double-buffered), so the device
 * never holds the whole file.  The result is independent of the store; free it with oem_text_result_destroy. */
int oem_assignment_text(oem_store *store, const double *counts, double display_thresh,
                        const uint8_t *names, const uint64_t *name_off, oem_text_result **out);
/* n_bytes of text, n_lines (= the store's reads), n_kept (= the sum of the lines' k); each may be NULL */
int oem_text_result_dims(const oem_text_result *r, uint64_t *n_bytes, uint64_t *n_lines, uint64_t *n_kept);
/* text: n_bytes; line_off (optional): n_lines + 1 byte offsets; kept (optional): n_lines u32, the k of each line */
int oem_text_result_copy(const oem_text_result *r, uint8_t *text, uint64_t *line_off, uint32_t *kept);
void oem_text_result_destroy(oem_text_result *r); /* NULL: no-op */

/* The `.prob.lz4` file (write_function.rs:243-263, 334-337): `prefix` followed by exactly the bytes oem_assignment_text
 * returns for the same arguments, as ONE complete LZ4 frame compressed on the device -- the text never leaves the
 * device uncompressed, and the caller links no LZ4 encoder.  prefix carries the file's header lines ("T\tR\n" and the
 * transcript names), so the result's text / n_bytes (oem_text_result_dims, _copy) are written to disk as they are;
 * prefix == NULL requires prefix_len == 0.  line_off and kept are what oem_assignment_text returns: offsets into the
 * body, after the prefix.
 * The frame: descriptor (FLG 0x78: version 01, independent blocks, block checksums, content size, no content
 * checksum; BD 0x40: blocks of at most 64 KiB), the blocks, the zero EndMark.  Any LZ4 frame decoder reads it.  It
 * departs from the file the reference's encoder writes (HC level 4, linked blocks, content checksum) in three ways:
 * blocks are independent (they compress in parallel), integrity is carried by per-block XXH32 checksums instead of a
 * content checksum (one serial chain over the whole content), and the parse is a fast greedy one, so the frame is
 * valid but larger than the reference's.  A block that does not shrink is stored raw; a chunk's last block may be
 * shorter than 64 KiB (legal anywhere in a frame).  The frame is a function of the content alone.
 * A store without reads gives a frame of the prefix alone; with an empty prefix as well that is the 15-byte
 * descriptor and the EndMark, which decodes to nothing.  Argument errors are those of oem_assignment_text plus the
 * NULL prefix with a length; all are reported before any device use, and *out is NULL after any failure. */
int oem_assignment_text_lz4(oem_store *store, const double *counts, double display_thresh,
                            const uint8_t *names, const uint64_t *name_off,
                            const uint8_t *prefix, uint64_t prefix_len, oem_text_result **out);
/* What a text result holds beyond its dims.  A result of oem_assignment_text answers CONTENT_BYTES with its n_bytes
 * and the other two with 0. */
#define OEM_TEXT_INFO_CONTENT_BYTES 1u /* the frame's content: prefix + body */
#define OEM_TEXT_INFO_BLOCKS 2u        /* blocks of the frame */
#define OEM_TEXT_INFO_RAW_BLOCKS 3u    /* ... of which stored uncompressed */
int oem_text_result_info(const oem_text_result *r, uint32_t key, uint64_t *value);

/* The `.count.mtx` file of the single-cell path (write_function.rs:53-54, through sprs::io::write_matrix_market):
 * `prefix` followed by one line per entry of the cells x transcripts matrix, in CSR order,
 *     "{row_base + cell + 1} {col + 1} {val}\n"
 * rows and columns 1-based, the f32 value as Rust's `{}` prints it: the shortest digits that read back as the same
 * f32, positional notation, no trailing ".0" (`1`, `0.1`, `16777216`, 1e30 as `1` and thirty zeros).  The matrix is the
 * CSR that oem_em_run_cells_sparse and the session return: cell_off has n_cells + 1 offsets (cell_off[0] = 0, never
 * decreasing; empty cells are fine), col / val have cell_off[n_cells] entries, every col is below n_txps.  prefix
 * carries the Matrix Market banner and the dimension line, so the result's text / n_bytes (oem_text_result_dims,
 * _copy) are the finished file; prefix == NULL requires prefix_len == 0.  row_base lets a rank that owns the cells
 * [row_base, row_base + n_cells) of a larger matrix produce its share of the body; row_base + n_cells may not exceed
 * 2^32 - 1.
 * The result: n_lines = n_kept = the number of entries, line_off the n_lines + 1 byte offsets of the lines into the body
 * (after the prefix), kept one per line; oem_text_result_info answers as for oem_assignment_text (CONTENT_BYTES =
 * n_bytes, 0 blocks).  No store is involved: the entries go up in chunks (8 B each), the text comes back; `device`
 * is the ordinal to run on.  All argument errors are reported before any device use, and *out is NULL after any
 * failure; without a device the call returns OEM_ERR_NO_DEVICE (there is no host fallback). */
int oem_count_matrix_text(const uint64_t *cell_off, uint32_t n_cells,
                          const uint32_t *col, const float *val,
                          uint32_t n_txps, uint32_t row_base,
                          const uint8_t *prefix, uint64_t prefix_len,
                          int device, oem_text_result **out);

/* The cells x transcripts matrix collapsed to cells x genes on the device (no counterpart in the reference, which
 * writes cells x transcripts only).  The input is the CSR that oem_em_run_cells_sparse and the sessions return
 * (cell_off: n_cells + 1 offsets from 0, never decreasing; col / val: cell_off[n_cells] entries, every col below
 * n_txps) and gene_of, one gene id below n_genes per transcript; gene_of need not be monotone and ids may be unused.
 * The rule, which the device is held to exactly:
 *   - for cell c and gene g the entries of cell c whose gene_of[col] is g are taken in CSR order, each converted to
 *     f64 and added one after the other starting from 0.0; the sum is rounded once to f32 (nearest-even, denormals
 *     kept);
 *   - cell c has an entry for gene g iff it has at least one entry of that gene -- there is no test on the value;
 *   - a cell's entries come in ascending gene id.
 * The result is an ordinary oem_cells_result (oem_cells_result_dims / _copy / _destroy): cell_off of n_cells + 1
 * entries, col the gene ids, val the sums, infos zero-filled; it is what oem_count_matrix_text takes, with n_genes in
 * the place of n_txps.  oem_cells_result_discard_tables on it returns OEM_ERR_STATE.  No cell may have more than 2^30
 * entries.  All argument errors are reported before any device use, and *out is NULL after any failure; without a
 * device the call returns OEM_ERR_NO_DEVICE (there is no host fallback). */
int oem_cells_gene_counts(const uint64_t *cell_off, uint32_t n_cells,
                          const uint32_t *col, const float *val,
                          const uint32_t *gene_of, uint32_t n_txps, uint32_t n_genes,
                          int device, oem_cells_result **out);

/* The `.quant` file of the bulk path (write_function.rs:104-120): `prefix` followed by one line per transcript,
 *     name '\t' len '\t' count '\n'
 * len in plain decimal, the f64 count as Rust's `{}` prints it: the shortest digits that read back as the same f64,
 * positional notation, never an exponent, no trailing ".0" (`1`, `0.1`, 1e23 as `1` and twenty-three zeros, 5e-324 as
 * `0.`, 323 zeros and `5`, -0.0 as `-0`; at most 327 bytes).  names / name_off: the transcript names as one byte blob
 * and n_txps + 1 offsets (name t = bytes [name_off[t], name_off[t+1])), as oem_assignment_text takes the read names;
 * lens and counts have n_txps entries.  prefix carries the header line "tname\tlen\tnum_reads\n", so the result's text /
 * n_bytes (oem_text_result_dims, _copy) are the finished file; prefix == NULL requires prefix_len == 0.
 * The result: n_lines = n_kept = n_txps, line_off the n_lines + 1 byte offsets of the lines into the body (after the
 * prefix), kept one per line; oem_text_result_info answers as for oem_assignment_text (CONTENT_BYTES = n_bytes, 0
 * blocks).  No store is involved: the columns go up in chunks, the text comes back; `device` is the ordinal to run on.
 * Argument errors -- a count that is not finite, name_off decreasing, a name that contains a tab or a newline, a NULL
 * array with n_txps > 0, a NULL out -- are reported before any device use, and *out is NULL after any failure.
 * n_txps == 0 is valid (the text is the prefix).  Without a device the call returns OEM_ERR_NO_DEVICE (there is no host
 * fallback). */
int oem_quant_text(const uint8_t *names, const uint64_t *name_off,
                   const uint64_t *lens, const double *counts, uint32_t n_txps,
                   const uint8_t *prefix, uint64_t prefix_len,
                   int device, oem_text_result **out);

/* The `.ambig_info.tsv` file (write_function.rs:122-145): `prefix` followed by one line per transcript,
 *     unique '\t' ambig '\t' total '\n',    ambig = total - unique, 0 where unique > total (saturating_sub)
 * from the two arrays oem_aux_counts returns (n_txps u32 each).  prefix carries the header line
 * "unique_reads\tambig_reads\ttotal_reads\n".  The result, the errors (a NULL array with n_txps > 0, a NULL prefix with a
 * length, a NULL out) and the behaviour without a device are those of oem_quant_text. */
int oem_ambig_text(const uint32_t *unique, const uint32_t *total, uint32_t n_txps,
                   const uint8_t *prefix, uint64_t prefix_len,
                   int device, oem_text_result **out);

/* --------------------------------------------------------------------- */
/* bootstrap                                                              */
/* --------------------------------------------------------------------- */

/* Device-side draw of one bootstrap resample in multiplicity form: the
 * Multinomial(n_reads; 1/n_reads ...) count vector of bootstrap.rs:7-16
 * (n draws from Uniform[0,n) with replacement; sorting is immaterial once
 * expressed as counts).  Counter-based (Philox4x32-10) stream keyed by
 * (seed, replica), a pure function of them and of the global read count n:
 *   counter block q < ceil(n/2) = (q & 0xffffffff, q >> 32, replica, 0x6f656d62),
 *   key = (seed & 0xffffffff, seed >> 32); draw 2q = (out[0] << 32) | out[1],
 *   draw 2q+1 = (out[2] << 32) | out[3] (draws with index >= n do not exist);
 *   a draw r selects read (r * n) >> 64.  A row shard keeps the counts of its
 *   own rows.  oracle/resample_np.py restates it; tests hold the kernel to it
 *   bit for bit.  out_row_w: n_reads u32 on the host. */
int oem_bootstrap_weights(oem_store *store, uint64_t seed, uint32_t replica, uint32_t *out_row_w);

/* em::bootstrap (em.rs:292-314): n_boot resampled EMs, each do_bootstrap
 * (em.rs:273-290) = do_em over random_sampling_iter with gate niter>50.
 *   row_w_all : optional n_boot x n_reads u32 (row-major) to inject the
 *               resamples (parity tests); NULL => drawn on the device as
 *               oem_bootstrap_weights(seed, b0 + b), b0 = OEM_OPT_BOOTSTRAP_FIRST_REPLICA
 *               (OEM_ERR_ARG if b0 + n_boot - 1 > 2^32 - 1).
 *   out       : n_boot x n_txps f64, row-major (replicate-major, as the
 *               Vec<Vec<f64>> of em.rs:292 / columns bootstrap.{i} of bulk.rs:181-193)
 *   infos     : optional, n_boot entries. */
int oem_bootstrap(oem_store *store, uint32_t n_boot, uint64_t seed, const uint32_t *row_w_all,
                  const double *init_abundances, uint32_t max_iter, double conv_thresh,
                  double *out, oem_run_info *infos);

/* --------------------------------------------------------------------- */
/* single-cell batch                                                      */
/* --------------------------------------------------------------------- */

/* The per-cell contract of single_cell.rs:139-160: every cell is an
 * independent em::em(&emi, 1) with init_abundances None, gate 50, over its
 * own reads.  Cells are given as one concatenated CSR (arrays as in
 * oem_store_create) plus cell_row_off[n_cells+1] (read offsets per cell);
 * out is n_cells x n_txps f64 row-major (the caller keeps entries > 0 as
 * (col u32, val f32) triplets, single_cell.rs:155-160). */
int oem_em_run_cells(const uint64_t *cell_row_off, uint32_t n_cells, const uint64_t *row_ptr,
                     const uint32_t *tid, const float *as_prob, const double *cov_prob,
                     uint64_t n_reads, uint64_t nnz, uint32_t n_txps, int device,
                     uint32_t max_iter, double conv_thresh, double *out, oem_run_info *infos);

/* Same inputs, validation and per-cell contract as oem_em_run_cells; the
 * result is the cells x transcripts matrix as CSR, in the exact form
 * single_cell.rs:151-160 writes: for cell c, entries [cell_off[c],
 * cell_off[c+1]) are the transcripts with count > 0.0 (f64 test), ascending
 * id, value (float)count rounded to nearest even.  Cells keep their input
 * order; a cell without reads has no entries.  The entries are picked out on
 * the device: host memory and read-back are proportional to the non-zeros,
 * not to n_cells x n_txps.  *out = NULL on any failure; release the result
 * with oem_cells_result_destroy. */
int oem_em_run_cells_sparse(const uint64_t *cell_row_off, uint32_t n_cells, const uint64_t *row_ptr,
                            const uint32_t *tid, const float *as_prob, const double *cov_prob,
                            uint64_t n_reads, uint64_t nnz, uint32_t n_txps, int device,
                            uint32_t max_iter, double conv_thresh, oem_cells_result **out);
int oem_cells_result_dims(const oem_cells_result *r, uint32_t *n_cells, uint64_t *n_entries);
/* cell_off: n_cells + 1; col, val: n_entries; infos: n_cells.  Any output may be NULL. */
int oem_cells_result_copy(const oem_cells_result *r, uint64_t *cell_off, uint32_t *col, float *val,
                          oem_run_info *infos);
void oem_cells_result_destroy(oem_cells_result *r); /* NULL: no-op */
/* single_cell.rs:117-160 from the built store on, in one call: the result equals oem_coverage_probs_cells_device on
 * the same cells, coordinates, bin_width, model and growth_rate, followed by oem_em_run_cells_sparse on that column --
 * but the column is computed, turned into the EM's weights and used on the device, one group of cells at a time.
 * Errors are those of the two calls, checked before any device work; an alignment outside its transcript is
 * OEM_ERR_STATE naming the first such cell.  out_cov_prob (nnz, optional): receives the column the EM used (NaN where
 * a zero-span alignment gives it, before the EM drops the read).  *out = NULL on any failure. */
int oem_em_run_cells_coverage_sparse(const uint64_t *cell_row_off, uint32_t n_cells, const uint64_t *row_ptr,
                                     const uint32_t *tid, const float *as_prob,
                                     const uint32_t *aln_start, const uint32_t *aln_end, const uint64_t *txp_len,
                                     uint64_t n_reads, uint64_t nnz, uint32_t n_txps,
                                     uint32_t bin_width, int model, double growth_rate,
                                     int device, uint32_t max_iter, double conv_thresh,
                                     double *out_cov_prob, oem_cells_result **out);

/* single_cell.rs:104-188 for all cells in one call: AlignmentFilters::filter over every cell's records into the cell's
 * own store, the per-cell coverage model if asked, em::em, the entries > 0.  records / group_off / n_groups are a
 * batch as oem_builder_add_groups takes it (group g = one read = records[group_off[g] .. group_off[g + 1])); cell c
 * owns the groups [cell_group_off[c], cell_group_off[c + 1]); cells without groups are allowed.  model: -1 no
 * coverage model, 0 logistic, 1 binomial (bin_width, growth_rate as in oem_em_run_cells_coverage_sparse).
 *
 * Per cell the result equals the long way round -- oem_builder_create(filters, txp_len, n_txps), oem_builder_add_groups
 * over that cell's groups only, oem_builder_export, then oem_em_run_cells_sparse (model -1) or
 * oem_em_run_cells_coverage_sparse (model 0 / 1) on the concatenation of the exports -- up to floating-point summation
 * order (which group of cells a cell lands in may change the tile layout, never the problem).  Exactly equal are:
 * out_kept (n_groups, optional), what add_groups returns for each group; table c of oem_cells_result_discard_tables,
 * that cell's builder's discard table.  A cell whose reads are all dropped has no entries and the oem_run_info of a
 * cell without reads.  The records are filtered on the device one group of cells at a time and the filtered CSR never
 * exists on the host; a group whose filter has to take the host loop (score_prob_denom not finite and positive, a gap
 * table above 2^22 entries, a mapped score beyond +-2^24: see oem_builder_add_groups_device) takes it, with the same
 * result.
 *
 * Argument errors are reported before any device use: those of oem_store_create_records (filters / txp_len NULL,
 * n_txps = 0, model, bin_width = 0 with a model, group_off NULL / not from 0 / decreasing, records NULL), those of the
 * cells calls, and cell_group_off NULL, not from 0, decreasing or not ending at n_groups.  A mapped record whose ref_id
 * is not below n_txps is OEM_ERR_ARG naming the cell and the first such record of the first such group of cells; an
 * alignment outside its transcript under a coverage model is OEM_ERR_STATE naming the cell.  Without a device:
 * OEM_ERR_NO_DEVICE.  *out = NULL on any failure. */
int oem_em_run_cells_records_sparse(const oem_filters *filters, const uint64_t *txp_len, uint32_t n_txps,
                                    const oem_aln_record *records, const uint64_t *group_off, uint64_t n_groups,
                                    const uint64_t *cell_group_off, uint32_t n_cells,
                                    uint32_t bin_width, int model, double growth_rate,
                                    int device, uint32_t max_iter, double conv_thresh,
                                    uint32_t *out_kept /* n_groups, or NULL */, oem_cells_result **out);
/* The per-cell DiscardTable of a result that came from records (oem_em_run_cells_records_sparse, a records session):
 * n_cells entries, in result order.  OEM_ERR_STATE for a result that did not; NULL arguments are OEM_ERR_ARG. */
int oem_cells_result_discard_tables(const oem_cells_result *r, oem_discard_table *out);

/* Collates the alignment records of cells by READ NAME, on the device: the first step of the reference's single-cell
 * worker (alignment_parser.rs:170-241, sort_and_parse_barcode_records), whose input is collated by barcode only.  What
 * it returns is the `group_off` / `cell_group_off` the records calls above take, once the caller has put its records
 * into `out_order` order.
 *
 * names / name_off: the n_records read names as one blob, record i's bytes at [name_off[i], name_off[i + 1]); name_off
 * starts at 0.  secondary: one byte per record, non-zero = the SAM secondary flag; NULL = no record has it.
 * cell_rec_off (n_cells + 1, from 0 to n_records, non-decreasing): cell c owns the records
 * [cell_rec_off[c], cell_rec_off[c + 1]); a cell may be empty.
 *
 * OEM_COLLATE_SORT.  For every cell, out_order[cell_rec_off[c] .. cell_rec_off[c + 1]) holds that cell's record indices
 * sorted by (1) the name as bytes, unsigned and lexicographic, a proper prefix first -- <[u8]>::cmp, what the
 * reference's x.name().cmp(&y.name()) does; (2) secondary != 0, so the primary comes first (:182-188); (3) the record
 * index.  The reference's sort is unstable and leaves the order among a read's secondaries open; (3) is the stable
 * choice, one of the orders its comparator allows.  out_group_off (capacity n_records + 1) receives the positions in
 * out_order where a new read starts -- a read is a maximal run of identical names inside one cell, so the same name in
 * two cells gives two groups (:201-239) -- and then n_records; *out_n_groups their number; out_cell_group_off
 * (n_cells + 1) the first group of every cell.
 * OEM_COLLATE_ADJACENT.  Nothing is sorted and out_order is the identity: a group ends where the name differs from the
 * previous record's or where a cell ends, the grouping of the bulk parser for name-collated input (:301-437).
 *
 * OEM_ERR_ARG before any device use: name_off, cell_rec_off or an output NULL, names NULL with n_records > 0, offsets
 * not from 0 or decreasing, cell_rec_off not ending at n_records, n_records > 2^32 - 1, a cell of more than 2^31 - 2
 * records, a mode that is none.  OEM_ERR_ARG found on the device, naming the first such record: an empty name (the
 * reference skips such records at :202; drop them before the call) and a name that contains a 0 byte (a BAM name
 * cannot; it is what lets the device compare zero-padded 8-byte keys).  The outputs are then unspecified.  Without a
 * device: OEM_ERR_NO_DEVICE.  The rule is oarfish_amd/csrc/oem_collate.h. */
#define OEM_COLLATE_SORT 0u
#define OEM_COLLATE_ADJACENT 1u
int oem_collate_names(const uint8_t *names, const uint64_t *name_off, const uint8_t *secondary /* or NULL */,
                      uint64_t n_records, const uint64_t *cell_rec_off, uint32_t n_cells,
                      uint32_t mode /* OEM_COLLATE_SORT, OEM_COLLATE_ADJACENT */, int device,
                      uint32_t *out_order, uint64_t *out_group_off, uint64_t *out_n_groups,
                      uint64_t *out_cell_group_off);

/* single_cell.rs:104-188 from its first step on, in one call: oem_collate_names and oem_em_run_cells_records_sparse
 * joined on the device.  records (n_records) and names / name_off / secondary are in the caller's INPUT order, collated
 * by barcode only; cell c owns the records [cell_rec_off[c], cell_rec_off[c + 1]).  mode, names, name_off, secondary and
 * cell_rec_off are oem_collate_names' arguments, the rest oem_em_run_cells_records_sparse's.
 *
 * The result is what the two calls give when the caller joins them -- oem_collate_names, the records put into
 * out_order order, oem_em_run_cells_records_sparse with the collation's group_off and cell_group_off -- but the order
 * is applied on the device, one group of cells at a time, and the caller neither waits for it nor gathers.  Exactly
 * equal to that join: out_order (n_records), out_group_off (capacity n_records + 1), *out_n_groups, out_cell_group_off
 * (n_cells + 1), out_kept (capacity n_records; *out_n_groups entries are written, one per group of the collated order)
 * and every table of oem_cells_result_discard_tables.  Each of the five outputs may be NULL.  The entries and infos are
 * equal as oem_em_run_cells_records_sparse states it: up to floating-point summation order.  Under
 * OEM_COLLATE_ADJACENT the order is the identity and nothing is moved.
 *
 * Argument errors are those of the two calls (oem_collate_names' on names, name_off, cell_rec_off, n_records, a cell's
 * size and mode; oem_em_run_cells_records_sparse's on filters, txp_len, n_txps, model and bin_width; records NULL with
 * n_records > 0), reported before any device use.  Found on the device: an empty name or a name with a 0 byte
 * (OEM_ERR_ARG naming the first such record of the first such group of cells); a mapped record whose ref_id is not
 * below n_txps (OEM_ERR_ARG naming the cell and the record's index in the caller's input order); an alignment outside
 * its transcript under a coverage model (OEM_ERR_STATE naming the cell).  Limits: n_records <= 2^32 - 1, a cell at most
 * 2^31 - 2 records.  Without a device: OEM_ERR_NO_DEVICE.  *out = NULL on any failure. */
int oem_em_run_cells_records_names_sparse(
    const oem_filters *filters, const uint64_t *txp_len, uint32_t n_txps,
    const oem_aln_record *records, uint64_t n_records,
    const uint8_t *names, const uint64_t *name_off, const uint8_t *secondary /* or NULL */,
    const uint64_t *cell_rec_off, uint32_t n_cells, uint32_t mode /* OEM_COLLATE_SORT, OEM_COLLATE_ADJACENT */,
    uint32_t bin_width, int model, double growth_rate, int device, uint32_t max_iter, double conv_thresh,
    uint32_t *out_order /* n_records, or NULL */, uint64_t *out_group_off /* n_records + 1, or NULL */,
    uint64_t *out_n_groups /* or NULL */, uint64_t *out_cell_group_off /* n_cells + 1, or NULL */,
    uint32_t *out_kept /* capacity n_records, *out_n_groups entries written; or NULL */,
    oem_cells_result **out);

/* Finds the CELLS of alignment records that are in any order, on the device.  The reference takes input in which all
 * records of a barcode are adjacent (single_cell.rs:196-213, alignment_parser.rs:244-299; docs/index.md: "all records of
 * a barcode must be adjacent"), which means a sort of the whole file by the CB tag before it starts.  This call lifts
 * that: it returns the permutation that collates the records by barcode and the cells' offsets in it, the
 * `cell_rec_off` oem_collate_names and oem_em_run_cells_records_names_sparse take.
 *
 * barcodes / barcode_off: the n_records barcodes as one blob, record i's bytes at [barcode_off[i], barcode_off[i + 1]);
 * barcode_off starts at 0.  Barcodes may differ in length.
 *
 * A cell is the set of records with one barcode, compared as bytes.  Cells are numbered in the order of their first
 * record in the input, so input that is barcode-collated already gives its cells in its own order.  Inside a cell the
 * records keep their input order.  out_order (n_records) is that cell-major permutation: out_order[k] is the input
 * index of the record at position k.  out_cell_rec_off (capacity n_records + 1; *out_n_cells + 1 entries are written)
 * holds every cell's first position and then n_records; *out_n_cells is the number of distinct barcodes.
 *
 * OEM_ERR_ARG before any device use: barcode_off or an output NULL, barcodes NULL with n_records > 0, offsets not from 0
 * or decreasing, n_records > 2^32 - 1 (and, in this version, n_records > 2^31 - 2: the barcodes are sorted as one batch
 * of oem_collate_names' sort).  OEM_ERR_ARG found on the device, naming the first such record: an empty barcode (the
 * reference bails when CB is missing, single_cell.rs:203, alignment_parser.rs:150) and a barcode that contains a 0
 * byte.  The outputs are then unspecified.  Without a device: OEM_ERR_NO_DEVICE.  The rule is
 * oarfish_amd/csrc/oem_collate.h. */
int oem_collate_barcodes(const uint8_t *barcodes, const uint64_t *barcode_off, uint64_t n_records, int device,
                         uint32_t *out_order            /* n_records */,
                         uint64_t *out_cell_rec_off     /* capacity n_records + 1; *out_n_cells + 1 written */,
                         uint64_t *out_n_cells);

/* single_cell.rs:104-188 from records in ANY order, in one call: oem_collate_barcodes and
 * oem_em_run_cells_records_names_sparse joined on the device.  records (n_records), barcodes / barcode_off, names /
 * name_off and secondary are in the caller's input order, one entry per record; nothing needs to be collated.  mode is
 * applied inside each cell, after the barcode collation.
 *
 * The result is what the caller gets by joining four steps: oem_collate_barcodes (order_bc, cell_rec_off); records,
 * names and secondary put into order_bc order on the host; oem_em_run_cells_records_names_sparse with that cell_rec_off
 * (order_names, ...); the two orders composed.  out_order[k] = order_bc[order_names[k]] is the caller's input index of
 * the record at position k of the final collated order.  Exactly equal to that join: out_order (n_records),
 * out_cell_rec_off (capacity n_records + 1) and *out_n_cells, out_group_off (capacity n_records + 1) and *out_n_groups,
 * out_cell_group_off (capacity n_records + 1; *out_n_cells + 1 written), out_kept (capacity n_records; *out_n_groups
 * written), every table of oem_cells_result_discard_tables and the entries' columns.  Each of the seven outputs may be
 * NULL.  The entries' values and the infos are equal as oem_em_run_cells_records_sparse states it: up to
 * floating-point summation order.
 *
 * The whole input is resident on the device during the call: 40 bytes a record, the names and their offsets, the
 * barcode order and one more offset a record; the barcode sort's buffers are released before the records go up, a
 * group's while it is collated.  Running out of device memory is OEM_ERR_OOM with everything released.
 *
 * Errors are those of the three calls.  Before any device use: theirs on filters, txp_len, n_txps, model, bin_width,
 * barcodes, barcode_off, names, name_off, n_records, mode; records NULL with n_records > 0.  Found on the device, all
 * OEM_ERR_ARG: an empty barcode or one with a 0 byte, naming the first such record; an empty name or one with a 0 byte,
 * naming the first such record of the input; a mapped record whose ref_id is not below n_txps, naming the cell and the
 * record's index in the caller's input order.  Limits: those of oem_collate_barcodes; a cell at most 2^31 - 2 records.
 * Without a device: OEM_ERR_NO_DEVICE.  *out = NULL on any failure. */
int oem_em_run_cells_records_barcodes_sparse(
    const oem_filters *filters, const uint64_t *txp_len, uint32_t n_txps,
    const oem_aln_record *records, uint64_t n_records,
    const uint8_t *barcodes, const uint64_t *barcode_off,
    const uint8_t *names, const uint64_t *name_off, const uint8_t *secondary /* or NULL */,
    uint32_t mode /* OEM_COLLATE_SORT, OEM_COLLATE_ADJACENT: applied inside each cell, after the barcode collation */,
    uint32_t bin_width, int model, double growth_rate, int device, uint32_t max_iter, double conv_thresh,
    uint32_t *out_order /* n_records, or NULL */,
    uint64_t *out_cell_rec_off /* capacity n_records + 1, or NULL */, uint64_t *out_n_cells /* or NULL */,
    uint64_t *out_group_off /* capacity n_records + 1, or NULL */, uint64_t *out_n_groups /* or NULL */,
    uint64_t *out_cell_group_off /* capacity n_records + 1, or NULL */,
    uint32_t *out_kept /* capacity n_records, or NULL */,
    oem_cells_result **out);

/* Marks the PCR DUPLICATES among the reads of a collated order, on the device.  The reference has no counterpart: its
 * documentation (docs/index.md:308-312) wants single-cell input "with already (UMI) deduplicated reads", because "a
 * count will be obtained for each read record", and names UMI counting as future work.  This call lifts that
 * requirement for input whose UB tags are corrected already; it is the composable step, as oem_collate_names is for
 * names.  The rule is oarfish_amd/csrc/oem_collate.h ("UMI deduplication"):
 *   - umis / umi_off: one UMI per INPUT record, as names are passed; a record without a UB tag has the empty string.
 *     flags: the records' OEM_REC_* words, or NULL (no record is unmapped).
 *   - order (n_positions), group_off (n_groups + 1; a group is a read) and cell_group_off (n_cells + 1) are a collated
 *     order as oem_collate_barcodes / oem_collate_names leave it: order[k] is the input index at position k.
 *   - head(g) = order[group_off[g]] (under OEM_COLLATE_SORT the read's primary); umi(g) is the UMI of record head(g), the
 *     UMIs of a read's other records are not examined.
 *   - group g takes part iff it has a record, umi(g) is not empty and record head(g) does not have OEM_REC_UNMAPPED.  A
 *     group that does not take part is never a duplicate and never shadows another.
 *   - inside one cell the groups that take part and whose UMIs are byte-identical (same length, same bytes) form a
 *     class; classes never span cells.  The class's smallest group index is its survivor, every other member a duplicate.
 *     Under OEM_COLLATE_SORT the survivor is the read whose name sorts first, whatever the input's order; under
 *     OEM_COLLATE_ADJACENT it is the first read in input order.
 * out_dup[g] is 0 or 1, out_survivor[g] the survivor's group index for a duplicate and g otherwise, out_cell_dups[c] the
 * number of duplicates in cell c.  Dropping the duplicate groups' positions from order / group_off / cell_group_off gives
 * the deduplicated collation; no cell becomes empty through it.
 *
 * Limits, on purpose: this call matches exactly, on corrected UMIs (umi_tools' `unique` method), and its key is (cell,
 * UMI), with no gene in it: oem_dedup_umis_rule below adds the gene and the one-mismatch correction.  In both the
 * survivor is not chosen by read length or by what the filter keeps.
 *
 * OEM_ERR_ARG before any device use: umi_off, group_off, cell_group_off or an output NULL; umis NULL while a UMI has
 * bytes; order NULL with n_positions > 0; offsets not from 0 or decreasing; group_off not ending at n_positions;
 * cell_group_off not ending at n_groups; n_records or n_positions > 2^32 - 1; a cell of more than 2^31 - 2 records or
 * groups.  OEM_ERR_ARG found on the device: an order entry that is not below n_records (naming the first such
 * position); a UMI that holds a 0 byte (naming the smallest such input index).  Empty UMIs are legal.  The cells are
 * taken in batches, as oem_collate_names takes them; the UMIs and flags of the whole input are resident during the
 * call.  Running out of device memory is OEM_ERR_OOM with everything released.  Without a device: OEM_ERR_NO_DEVICE. */
int oem_dedup_umis(const uint8_t *umis, const uint64_t *umi_off, const uint32_t *flags /* n_records, or NULL */,
                   uint64_t n_records, const uint32_t *order, uint64_t n_positions,
                   const uint64_t *group_off, uint64_t n_groups, const uint64_t *cell_group_off, uint32_t n_cells,
                   int device,
                   uint8_t *out_dup          /* n_groups */,
                   uint64_t *out_survivor    /* n_groups */,
                   uint64_t *out_cell_dups   /* n_cells */);

/* oem_em_run_cells_records_barcodes_sparse with UMI deduplication: cells from raw records in one call.  The arguments
 * are that call's, with umis / umi_off (one UMI per input record, as oem_dedup_umis takes them) added; the records'
 * own flags words say which are unmapped.  Per group of cells the duplicates leave the collation on the device, between
 * the name collation and the record gather: a duplicate's records are never gathered, filtered or counted.
 *
 * The result is what the caller gets by joining seven steps: oem_collate_barcodes (order_bc, cell_rec_off); records,
 * names and secondary put into order_bc order on the host; oem_collate_names with that cell_rec_off (order_names,
 * group_off, cell_group_off); the composed order, order[k] = order_bc[order_names[k]]; oem_dedup_umis on it with the
 * caller's umis and the records' flags; the duplicate groups' positions dropped on the host (order', group_off',
 * cell_group_off', cell_rec_off'); oem_em_run_cells_records_sparse on records[order'] with group_off' and
 * cell_group_off'.  The seven outputs of the barcodes call describe that DEDUPLICATED collation: *out_n_survivors
 * positions of out_order are written, out_cell_rec_off counts positions of it, *out_n_groups reads remain.  Exactly
 * equal to that join: every index array and count, out_kept, every table of oem_cells_result_discard_tables (a
 * duplicate is in no table), out_cell_dups (capacity n_records; *out_n_cells written: the duplicates dropped from every
 * cell) and the entries' columns.  Each output but `out` may be NULL.  The entries' values and the infos are equal as
 * oem_em_run_cells_records_sparse states it: up to floating-point summation order.  With every UMI empty the call
 * gives oem_em_run_cells_records_barcodes_sparse's result exactly, and no duplicate.
 *
 * Resident on the device beyond what the barcodes call holds: the UMI blob and 8 bytes of offsets per record; a group's
 * UMI collation is released before its records are gathered.  Running out of device memory is OEM_ERR_OOM with
 * everything released.
 *
 * Errors are those of the barcodes call and of oem_dedup_umis.  Before any device use also: umi_off NULL, not from 0 or
 * decreasing; umis NULL while a UMI has bytes.  Found on the device also: a UMI that holds a 0 byte, OEM_ERR_ARG naming
 * the smallest such input index.  A mapped record whose ref_id is not below n_txps is found among the survivors only,
 * and named by its cell and its index in the caller's input order.  Without a device: OEM_ERR_NO_DEVICE.  *out = NULL
 * on any failure. */
int oem_em_run_cells_records_umis_sparse(
    const oem_filters *filters, const uint64_t *txp_len, uint32_t n_txps,
    const oem_aln_record *records, uint64_t n_records,
    const uint8_t *barcodes, const uint64_t *barcode_off,
    const uint8_t *names, const uint64_t *name_off, const uint8_t *secondary /* or NULL */,
    const uint8_t *umis, const uint64_t *umi_off,
    uint32_t mode /* OEM_COLLATE_SORT, OEM_COLLATE_ADJACENT: applied inside each cell, after the barcode collation */,
    uint32_t bin_width, int model, double growth_rate, int device, uint32_t max_iter, double conv_thresh,
    uint32_t *out_order /* capacity n_records, *out_n_survivors written; or NULL */, uint64_t *out_n_survivors /* or NULL */,
    uint64_t *out_cell_rec_off /* capacity n_records + 1, or NULL */, uint64_t *out_n_cells /* or NULL */,
    uint64_t *out_group_off /* capacity n_records + 1, or NULL */, uint64_t *out_n_groups /* or NULL */,
    uint64_t *out_cell_group_off /* capacity n_records + 1, or NULL */,
    uint32_t *out_kept /* capacity n_records, or NULL */,
    uint64_t *out_cell_dups /* capacity n_records, *out_n_cells written; or NULL */,
    oem_cells_result **out);

/* A UMI RULE: gene-aware keys and one-mismatch correction for the two calls above.  The reference has no counterpart
 * (docs/index.md:308-312 wants deduplicated input); the rule is oarfish_amd/csrc/oem_collate.h ("UMI deduplication"),
 * whose host walk is the specification the device is held to exactly.
 *   - gene_of: NULL, or one gene id per transcript (n_txps of them).  gene(g) = gene_of[ref_id(head(g))], the gene of the
 *     read's first record in collated order; 0 for every group when gene_of is NULL.  A segment is the groups of one cell
 *     that take part and share gene(g); a class is the groups of one SEGMENT with byte-identical UMIs, so the same UMI in
 *     two genes of one cell is two molecules (Cell Ranger, alevin-fry and UMI-tools key by (cell, gene, UMI)).
 *   - correct: 0 or 1.  With 1, two classes of one segment whose UMIs have the same length and differ in exactly one
 *     byte position are neighbours (any bytes; there is no alphabet); a class u takes as its parent the neighbour v with
 *     n(v) > n(u) that has the most groups, among equals the one whose UMI bytes compare smallest; parents are chosen
 *     from the original counts, a root is a class without a parent, and a molecule is the groups of all classes with one
 *     root.  Its smallest group index survives, every other member is a duplicate of it.  A corrected group is one
 *     whose class has a parent; it may itself be its molecule's survivor.
 * rule == NULL or {NULL, 0, 0} gives oem_dedup_umis / oem_em_run_cells_records_umis_sparse exactly.
 * Limits, on purpose: the gene of a read that maps to several genes is its head's; one mismatch only, no indels; the
 * survivor is not chosen by read length or by what the filter keeps; deduplication still runs before the filter.  The
 * UMI sessions take the same rule through oem_cells_stream_set_umi_rule. */
typedef struct {
    const uint32_t *gene_of; /* n_txps gene ids, or NULL: no gene in the key */
    uint32_t n_txps;
    uint32_t correct;        /* 0: exact matching; 1: one-mismatch correction */
} oem_umi_rule;

/* oem_dedup_umis under a rule.  ref_id (n_records): the records' transcript ids, required iff rule->gene_of is given and
 * read only at the heads of groups that take part (an unmapped record's ref_id is never looked at).
 * out_cell_corrected[c] (or NULL) is the number of corrected groups of cell c.  OEM_ERR_ARG before any device use, beyond
 * oem_dedup_umis': gene_of given and n_txps == 0; gene_of given and ref_id NULL; correct > 1.  Found on the device also:
 * the head of a group that takes part whose ref_id is not below n_txps, naming the smallest such input index. */
int oem_dedup_umis_rule(const oem_umi_rule *rule /* or NULL */,
                        const uint8_t *umis, const uint64_t *umi_off, const uint32_t *flags /* n_records, or NULL */,
                        const uint32_t *ref_id /* n_records, or NULL */,
                        uint64_t n_records, const uint32_t *order, uint64_t n_positions,
                        const uint64_t *group_off, uint64_t n_groups, const uint64_t *cell_group_off, uint32_t n_cells,
                        int device,
                        uint8_t *out_dup            /* n_groups */,
                        uint64_t *out_survivor      /* n_groups */,
                        uint64_t *out_cell_dups     /* n_cells */,
                        uint64_t *out_cell_corrected /* n_cells, or NULL */);

/* oem_em_run_cells_records_umis_sparse under a rule: the join of its seven steps with oem_dedup_umis_rule in place of
 * oem_dedup_umis, the records' own ref_id words being the ref_id; exactly equal to that join as the umis call is to
 * its own.  rule->gene_of, when given, must have rule->n_txps == n_txps.  out_cell_corrected (capacity n_records,
 * *out_n_cells written; or NULL): the corrected groups of every cell.  A head of a read that takes part whose ref_id is
 * not below n_txps is OEM_ERR_ARG found on the device, naming the record by its input index. */
int oem_em_run_cells_records_umis_rule_sparse(
    const oem_umi_rule *rule /* or NULL */,
    const oem_filters *filters, const uint64_t *txp_len, uint32_t n_txps,
    const oem_aln_record *records, uint64_t n_records,
    const uint8_t *barcodes, const uint64_t *barcode_off,
    const uint8_t *names, const uint64_t *name_off, const uint8_t *secondary /* or NULL */,
    const uint8_t *umis, const uint64_t *umi_off,
    uint32_t mode, uint32_t bin_width, int model, double growth_rate, int device, uint32_t max_iter, double conv_thresh,
    uint32_t *out_order /* capacity n_records, *out_n_survivors written; or NULL */, uint64_t *out_n_survivors /* or NULL */,
    uint64_t *out_cell_rec_off /* capacity n_records + 1, or NULL */, uint64_t *out_n_cells /* or NULL */,
    uint64_t *out_group_off /* capacity n_records + 1, or NULL */, uint64_t *out_n_groups /* or NULL */,
    uint64_t *out_cell_group_off /* capacity n_records + 1, or NULL */,
    uint32_t *out_kept /* capacity n_records, or NULL */,
    uint64_t *out_cell_dups /* capacity n_records, *out_n_cells written; or NULL */,
    uint64_t *out_cell_corrected /* capacity n_records, *out_n_cells written; or NULL */,
    oem_cells_result **out);

/* A BARCODE RULE: raw cell barcodes (CR tags) matched against a whitelist, with one-mismatch correction.  The reference
 * has no counterpart: it wants every record to carry a CORRECTED cell barcode (docs/index.md:308-312), and every other
 * barcode entry point here compares barcodes as bytes, so that a barcode with one sequencing error would be a cell of its
 * own.  The rule is oarfish_amd/csrc/oem_barcode_correct.h, whose host walk is the specification the device is held to
 * exactly.
 *   - labels / label_off: the whitelist (the chemistry's permit list), n_labels >= 1 distinct labels of 1 .. 64 bytes as
 *     one blob with n_labels + 1 offsets from 0; a record's id is its label's index.
 *   - alphabet: NULL for "ACGT", or n_alphabet (1 .. 8) distinct non-zero bytes.
 *   - exact: a barcode that is byte-identical to label w has id = w and OEM_BARCODE_EXACT.  n(w) is the number of records
 *     of the call that are exact for w, whatever their flags; a corrected record never adds to it.
 *   - neighbours of a non-empty barcode b that is not exact: the labels of b's length that differ from b in exactly one
 *     byte position AND whose byte at that position is in the alphabet.  b's own byte there may be anything (an N is
 *     handled, two Ns have no neighbour); a label byte outside the alphabet is only ever matched exactly.
 *   - no neighbour: OEM_BARCODE_NO_NEIGHBOUR.  multi = 0 (STARsolo's 1MM): exactly one neighbour gives
 *     OEM_BARCODE_CORRECTED to it, more than one OEM_BARCODE_AMBIGUOUS.  multi = 1: one neighbour gives
 *     OEM_BARCODE_CORRECTED to it whatever its n; of several the one whose n(w) is strictly largest wins, a tie for the
 *     largest is OEM_BARCODE_AMBIGUOUS.
 *   - an empty barcode (no tag) is OEM_BARCODE_MISSING: not the error it is for the calls that take corrected barcodes.
 *   - NO_NEIGHBOUR, AMBIGUOUS and MISSING records are REJECTED: id = OEM_BARCODE_NO_ID, and they belong to no cell.
 *   - a cell is the accepted records of one label.  Cells are numbered by their first accepted record in input order and
 *     records keep input order inside a cell: oem_collate_barcodes' numbering, so input that holds only whitelisted
 *     barcodes gives exactly that call's order / cell_rec_off.  A cell's label is the whitelist's bytes, labels[id of the
 *     cell's first record], not any record's.
 * The result never depends on a hash, on probe order or on the arrival order of atomics.  Limits, on purpose: no base
 * qualities (Cell Ranger's posterior needs them), no indels, no knee.  The any-order barcoded session takes the rule
 * through oem_cells_stream_set_whitelist. */
typedef struct {
    const uint8_t *labels; const uint64_t *label_off; uint32_t n_labels;
    uint32_t multi;            /* 0, 1 */
    const uint8_t *alphabet;   /* NULL: "ACGT" */
    uint32_t n_alphabet, reserved;
} oem_barcode_rule;

#define OEM_BARCODE_EXACT 0
#define OEM_BARCODE_CORRECTED 1
#define OEM_BARCODE_NO_NEIGHBOUR 2
#define OEM_BARCODE_AMBIGUOUS 3
#define OEM_BARCODE_MISSING 4
#define OEM_BARCODE_NO_ID 0xffffffffu

/* The composable step, as oem_collate_barcodes is for corrected barcodes: the rule above on the device.  barcodes /
 * barcode_off: one raw barcode per record, as oem_collate_barcodes takes them, the empty string where the tag is missing.
 * out_id (n_records) and out_status (n_records): every record's label and OEM_BARCODE_* code.  out_order (capacity
 * n_records; *out_n_accepted entries are written) and out_cell_rec_off (capacity n_records + 1; *out_n_cells + 1 entries
 * are written) are the cells of the accepted records, positions counting accepted records only.  out_counts (5): the
 * records of every status code.  Any output but the two scalars may be NULL.
 *
 * OEM_ERR_ARG before any device use: rule, labels or label_off NULL; n_labels == 0; label_off not from 0 or decreasing; an
 * empty label; a label of more than 64 bytes; multi > 1; an alphabet that is empty, longer than 8 bytes or holds a
 * repeated or a 0 byte; barcode_off, out_n_cells or out_n_accepted NULL; oem_collate_barcodes' checks and limits on
 * barcodes, barcode_off and n_records.  OEM_ERR_ARG found on the device, in this order: a label that holds a 0 byte
 * (naming the smallest such label); two equal labels (naming i < j, the smallest pair with i first, i being the first
 * label with those bytes); a barcode that holds a 0 byte (naming the smallest such record).  The outputs are then
 * unspecified.  Resident during the call: the whitelist (its labels and 4 bytes a slot of a table of at least 2
 * n_labels slots, 4 bytes a label of counts), the barcodes, and 13 bytes a record.  Running out of device memory is
 * OEM_ERR_OOM with everything released.  Without a device: OEM_ERR_NO_DEVICE. */
int oem_correct_barcodes(const oem_barcode_rule *rule,
                         const uint8_t *barcodes, const uint64_t *barcode_off, uint64_t n_records, int device,
                         uint32_t *out_id            /* n_records, or NULL */,
                         uint8_t *out_status         /* n_records, or NULL */,
                         uint32_t *out_order         /* capacity n_records, *out_n_accepted written; or NULL */,
                         uint64_t *out_cell_rec_off  /* capacity n_records + 1, *out_n_cells + 1 written; or NULL */,
                         uint64_t *out_n_cells, uint64_t *out_n_accepted,
                         uint64_t *out_counts        /* 5, indexed by OEM_BARCODE_*; or NULL */);

/* oem_em_run_cells_records_umis_rule_sparse on RAW barcodes: from a sequencer's records to the cells' counts in one
 * call.  The arguments and outputs are that call's, with the barcode rule in front; umis / umi_off may both be NULL,
 * meaning no deduplication (umi_rule is then checked and otherwise unused).  Three outputs are added: out_wl_id
 * (n_records) and out_status (n_records) as oem_correct_barcodes gives them, and out_counts (5).
 *
 * The result is what the caller gets by joining five steps: oem_correct_barcodes; the rejected records dropped on the
 * host from records, names, secondary and umis; the accepted records given their labels' bytes as barcodes;
 * oem_em_run_cells_records_umis_rule_sparse on that input (with every UMI empty where umis is NULL); its out_order mapped
 * back to the caller's input indices.  Exactly equal to that join: every index array and count, out_kept, every table of
 * oem_cells_result_discard_tables, out_cell_dups, out_cell_corrected and the entries' columns; the entries' values and
 * the infos are equal as that call states it.  out_order holds indices of the CALLER's input; *out_n_survivors, the
 * capacities and the offsets count accepted records only.  Input that is rejected entirely gives zero cells and an empty
 * result, not an error.
 *
 * A REJECTED RECORD'S NAME, UMI AND ref_id ARE NEVER LOOKED AT: the rejected records go up with the rest and are never
 * gathered, so an empty name, a 0 byte in a name or UMI, or a ref_id that is not below n_txps is no error on a rejected
 * record.  On an accepted record they are the errors of the umis call, found on the device and naming the record by its
 * index in the caller's input.  Errors otherwise: oem_correct_barcodes' on the rule and the barcodes, then that call's.
 * Resident beyond what that call holds: the whitelist and 5 bytes a record while the cells are found.  *out = NULL on any
 * failure. */
int oem_em_run_cells_records_whitelist_sparse(
    const oem_barcode_rule *rule,
    const oem_umi_rule *umi_rule /* or NULL */,
    const oem_filters *filters, const uint64_t *txp_len, uint32_t n_txps,
    const oem_aln_record *records, uint64_t n_records,
    const uint8_t *barcodes, const uint64_t *barcode_off,
    const uint8_t *names, const uint64_t *name_off, const uint8_t *secondary /* or NULL */,
    const uint8_t *umis /* or NULL */, const uint64_t *umi_off /* or NULL */,
    uint32_t mode, uint32_t bin_width, int model, double growth_rate, int device, uint32_t max_iter, double conv_thresh,
    uint32_t *out_order /* capacity n_records, *out_n_survivors written; or NULL */, uint64_t *out_n_survivors /* or NULL */,
    uint64_t *out_cell_rec_off /* capacity n_records + 1, or NULL */, uint64_t *out_n_cells /* or NULL */,
    uint64_t *out_group_off /* capacity n_records + 1, or NULL */, uint64_t *out_n_groups /* or NULL */,
    uint64_t *out_cell_group_off /* capacity n_records + 1, or NULL */,
    uint32_t *out_kept /* capacity n_records, or NULL */,
    uint64_t *out_cell_dups /* capacity n_records, *out_n_cells written; or NULL */,
    uint64_t *out_cell_corrected /* capacity n_records, *out_n_cells written; or NULL */,
    uint32_t *out_wl_id /* n_records, or NULL */,
    uint8_t *out_status /* n_records, or NULL */,
    uint64_t *out_counts /* 5, or NULL */,
    oem_cells_result **out);

/* The bulk parser and oem_store_create_records in one call: parse_alignments (alignment_parser.rs:301-437) from the
 * records and read names as a BAM reader produces them, in input order, to the resident store.  records (n_records),
 * names / name_off and secondary are oem_collate_names' per-record arrays; the rule is oarfish_amd/csrc/oem_collate.h
 * (the bulk parser):
 *   - a record with OEM_REC_UNMAPPED takes no part (:367-370): it cuts no read, its name is never looked at (it may be
 *     empty or hold a 0 byte), and a read made only of such records is no group, so no `no_mapping` entry either.
 *     (oem_aln_record has no "mapped, but without a reference id" state, :377 and :410: nothing corresponds to it.)
 *   - OEM_COLLATE_ADJACENT is the reference's parser: the surviving records in input order, a read a maximal run of
 *     identical names among them (`A, unmapped, A` is one read of two).  OEM_COLLATE_SORT lifts the requirement that the
 *     input be name-collated: the surviving records are sorted by oem_collate_names' rule as one cell, then cut.
 *   - under OEM_COLLATE_ADJACENT with sort_check_num = N > 0 (--sort-check-num, prog_opts.rs:558-561, 100 000 there) the
 *     first min(N, n_groups) groups are checked as at :396-408: if a checked group has the name of an earlier group the
 *     call fails with OEM_ERR_STATE, naming the smallest such group, the input index of its first record, that of the
 *     earlier group's first record, and that OEM_COLLATE_SORT accepts such input.  A repeat at a group index >= N is
 *     accepted, as by the reference; N = 0 is no check; under OEM_COLLATE_SORT there is nothing to check.
 *   - the filter is oem_store_create_records', over the groups in order; row r of the store is the r-th group with
 *     out_kept > 0 and its name the name of the first record of that group (name_vec, :341-351).
 *
 * The call gives what the caller gets by joining these steps by hand: drop the unmapped records, their names and flags
 * on the host; oem_collate_names on what is left as ONE cell (cell_rec_off = {0, n_parsed}); the records put into that
 * order; oem_store_create_records with the collation's group_off and the same opts, model, bin_width and growth_rate.
 * Exactly equal to that join, for every weight_coding and both layout_build values: out_order mapped back to input
 * indices (n_parsed entries: out_order[k] is the caller's index of the record at position k), out_group_off
 * (n_groups + 1 entries), out_kept (n_groups), the discard table, every field of out_info and the row names
 * (out_row_name_off: n_reads + 1 offsets from 0 into out_row_names).  The store is that store: its weights are
 * bit-identical, EM results agree as oem_store_create_records states for its own long way round.  Every output but `out`
 * may be NULL, out_row_names and out_row_name_off only together.
 *
 * oem_parse_info: n_unmapped records skipped, n_parsed = n_records - n_unmapped, n_groups reads among them, n_reads
 * rows of the store, unique_alignments = groups with out_kept == 1 (:386-388), n_checked groups the collation check
 * looked at.
 *
 * The whole input is resident on the device until the filter has run: 40 bytes a record, the names and 8 bytes of
 * offsets a record (the records twice for the length of their gather), 4 more bytes a record when there are unmapped
 * records; the collation holds about 150 bytes a surviving record while it runs and releases them before the records
 * are gathered.  Running out of device memory is OEM_ERR_OOM with everything released.
 *
 * Errors.  Before any device use, OEM_ERR_ARG: those of oem_store_create_records on filters, txp_len, n_txps, model,
 * bin_width and opts; those of oem_collate_names on names, name_off and mode; records NULL with n_records > 0; one of
 * out_row_names / out_row_name_off without the other; n_records > 2^31 - 2 (one collation batch).  Found on the device:
 * a surviving record with an empty name or a 0 byte in its name (OEM_ERR_ARG naming the first such record by its input
 * index); the collation check (OEM_ERR_STATE, above); a mapped record whose ref_id is not below n_txps (OEM_ERR_ARG
 * naming the input index); an alignment outside its transcript under a coverage model (OEM_ERR_STATE); 2^32 or more
 * kept alignments (OEM_ERR_ARG).  The host loop takes the groups, with the same result, when
 * oem_builder_add_groups_device's would.  Without a device: OEM_ERR_NO_DEVICE.  *out = NULL on any failure; the other
 * outputs are then unspecified. */
typedef struct {
    uint64_t n_unmapped, n_parsed, n_groups, n_reads, unique_alignments, n_checked, reserved[2];
} oem_parse_info;
int oem_store_create_records_names(
    const oem_filters *filters, const uint64_t *txp_len, uint32_t n_txps,
    const oem_aln_record *records, uint64_t n_records,
    const uint8_t *names, const uint64_t *name_off, const uint8_t *secondary /* or NULL */,
    uint32_t mode /* OEM_COLLATE_SORT, OEM_COLLATE_ADJACENT */, uint64_t sort_check_num,
    uint32_t bin_width, int model, double growth_rate, int device, const oem_store_opts *opts,
    uint32_t *out_order          /* capacity n_records; n_parsed written; or NULL */,
    uint64_t *out_group_off      /* capacity n_records + 1; n_groups + 1 written; or NULL */,
    uint32_t *out_kept           /* capacity n_records; n_groups written; or NULL */,
    uint8_t *out_row_names       /* capacity name_off[n_records]; or NULL */,
    uint64_t *out_row_name_off   /* capacity n_records + 1; n_reads + 1 written; or NULL (together with out_row_names) */,
    oem_discard_table *out_discard /* or NULL */, oem_parse_info *out_info /* or NULL */,
    oem_store **out);

/* A per-cell SESSION: the caller pushes cells one by one, from any number of threads, as they become available
 * (single_cell.rs:96-193: N workers each pop one cell and build its private store).  The library stages the cells,
 * cuts them into groups, runs every group through the batched per-cell driver while later cells still arrive, and
 * hands back one sparse result at the end.  One device per session. */
typedef struct oem_cells_stream oem_cells_stream;

typedef struct {
    uint32_t n_txps;
    int32_t  device;
    uint32_t max_iter;        /* as oem_em_run_cells */
    double   conv_thresh;
    uint32_t coverage;        /* 0: no coverage model (w = as_prob); 1: the per-cell coverage model from the pushed
                                 coordinates, as oem_em_run_cells_coverage_sparse */
    uint32_t bin_width;       /* coverage = 1 only, with model / growth_rate as in that call */
    int32_t  model;
    double   growth_rate;
    uint64_t group_nnz;       /* 0 = default: a group is started once this many alignments are staged ... */
    uint32_t group_cells;     /* 0 = default: ... or this many cells; the limits of oem_em_run_cells' own group rule
                                 (transcript space < 2^32, 65 535 cells, tile x bucket table) always apply */
    uint64_t max_staged_nnz;  /* 0 = default: push blocks while more than this is staged and not yet on the device */
    uint32_t reserved[4];     /* 0 */
} oem_cells_stream_opts;

#define OEM_CELLS_STREAM_INFO_CELLS 1u                /* cells accepted */
#define OEM_CELLS_STREAM_INFO_ALIGNMENTS 2u           /* alignments accepted */
#define OEM_CELLS_STREAM_INFO_GROUPS 3u               /* groups a device worker has started */
#define OEM_CELLS_STREAM_INFO_GROUPS_BEFORE_FINISH 4u /* ... of these, before oem_cells_stream_finish was called:
                                                         above 0, arrival and compute overlapped */
#define OEM_CELLS_STREAM_INFO_BLOCKED_US 5u           /* microseconds pushes spent blocked on back-pressure, summed
                                                         over the pushing threads */
#define OEM_CELLS_STREAM_INFO_GROUPS_BATCHED 6u       /* groups that ran as one batched store (the others: cell by cell) */
/* an any-order barcoded session (oem_cells_stream_set_barcodes_any_order); 0 on every other session */
#define OEM_CELLS_STREAM_INFO_ARENA_BYTES 7u          /* the most device memory the arena of survivors held, in bytes (a
                                                         growing array is counted twice while it is copied, and so is
                                                         the arena while finish lays it out by cell) */
#define OEM_CELLS_STREAM_INFO_BARCODE_MISSES 8u       /* survivors that missed the first lookup of their batch */
#define OEM_CELLS_STREAM_INFO_BARCODE_TABLE_SLOTS 9u  /* the barcode table's capacity (after finish: the final one) */
/* a UMI session (oem_cells_stream_set_umis); 0 on every other session */
#define OEM_CELLS_STREAM_INFO_UMI_DUP_READS 10u       /* reads dropped as duplicates, in groups that have run */
#define OEM_CELLS_STREAM_INFO_UMI_DUP_RECORDS 11u     /* their records */
#define OEM_CELLS_STREAM_INFO_UMI_CORRECTED_READS 12u /* reads corrected under a rule with correct (oem_cells_stream_set_umi_rule),
                                                         in groups that have run */
/* a whitelist session (oem_cells_stream_set_whitelist); 0 on every other session */
#define OEM_CELLS_STREAM_INFO_BARCODE_REJECTED 13u    /* mapped records dropped by the barcode rule, in their batch or at finish */
#define OEM_CELLS_STREAM_INFO_BARCODE_DEFERRED 14u    /* records whose choice between several neighbours waited for finish */

/* Argument errors (n_txps = 0, opts or out NULL, coverage = 1 without txp_len, with bin_width = 0 or with a model
 * other than 0 / 1, a non-zero reserved word) are reported before any device is touched; without a device the call
 * returns OEM_ERR_NO_DEVICE.  txp_len (n_txps entries) is copied; it is not read with coverage = 0.  *out = NULL on
 * any failure. */
int oem_cells_stream_create(const oem_cells_stream_opts *opts, const uint64_t *txp_len, oem_cells_stream **out);
/* One cell: its own CSR (row_ptr: n_reads + 1 entries starting at 0; tid, as_prob: nnz) and, with coverage = 1, its
 * alignments' coordinates (NULL otherwise).  Thread-safe.  The cell is checked on the calling thread (row_ptr[0] = 0,
 * non-decreasing, row_ptr[n_reads] = nnz, every tid < n_txps, coordinates present under coverage = 1) and its arrays
 * are copied: the caller may free them on return.  *out_ticket (optional) receives the cell's ticket: 0, 1, 2 ... in
 * the order in which pushes were accepted; cell k of the result is the cell with ticket k.  A cell without reads is
 * allowed.  An argument error (OEM_ERR_ARG) rejects that cell only: no ticket is used up and the session stays
 * usable.  The call blocks while more than max_staged_nnz alignments are staged and not yet on the device, except that
 * a cell larger than that budget is accepted when nothing else is staged.  A device or allocation failure in a group
 * is sticky: every later push and finish returns that status and its message.  After finish: OEM_ERR_STATE. */
int oem_cells_stream_push(oem_cells_stream *s, const uint64_t *row_ptr, const uint32_t *tid, const float *as_prob,
                          const uint32_t *aln_start, const uint32_t *aln_end, uint64_t n_reads, uint64_t nnz,
                          uint64_t *out_ticket);
/* Turns a fresh session (no cell pushed yet) into a RECORDS session: cells are then pushed as their alignment records
 * (oem_cells_stream_push_records) and filtered on the device, as oem_em_run_cells_records_sparse does; with
 * coverage = 1 the coverage model runs on the filter's coordinates.  filters and txp_len (n_txps entries) are copied.
 * NULL arguments: OEM_ERR_ARG.  Once a cell has been pushed, or after finish: OEM_ERR_STATE.  On a records session
 * oem_cells_stream_push returns OEM_ERR_STATE; on a plain one oem_cells_stream_push_records does. */
int oem_cells_stream_set_filters(oem_cells_stream *s, const oem_filters *filters, const uint64_t *txp_len);
/* One cell of a records session: its reads' records as a batch (group_off: n_groups + 1 entries from 0).  In every
 * other respect as oem_cells_stream_push: thread-safe; checked on the calling thread (group_off from 0 and not
 * decreasing, records present; an argument error rejects that cell only and uses no ticket); the arrays are copied,
 * into page-locked staging, 40 B per record; tickets are issued the same way; the same back-pressure, its budget
 * (max_staged_nnz, group_nnz) counted in records; the same sticky device errors.  A ref_id that is not below n_txps is
 * found on the device: it fails the group, is sticky and names the cell's ticket ("cell <ticket>") and the record's
 * index within its group of cells.  After finish, oem_cells_result_discard_tables gives the cells' tables. */
int oem_cells_stream_push_records(oem_cells_stream *s, const oem_aln_record *records, const uint64_t *group_off,
                                  uint64_t n_groups, uint64_t *out_ticket);
/* A BARCODED session: oem_em_run_cells_records_names_sparse for a caller that never holds the whole input and has not
 * cut it into cells (the reference's single-cell reader, single_cell.rs:196-227 with alignment_parser.rs:244-299,
 * walks a barcode-collated BAM record by record and cuts a cell where the CB tag changes, while workers sort and run
 * the cells behind it).  oem_cells_stream_set_barcodes turns a fresh RECORDS session (after
 * oem_cells_stream_set_filters, before any push) into one; `mode` is the name rule applied inside every cell
 * (oem_collate_names).  A mode that is neither: OEM_ERR_ARG.  On a plain session, after a push, after finish, or a
 * second time: OEM_ERR_STATE.
 *
 * The rule (oarfish_amd/csrc/oem_collate.h, "Cells from a barcode-collated stream").  The session's input is its
 * accepted batches concatenated in ticket order; a record's session-global index counts all records of that input,
 * 64 bits, unmapped ones included.
 *   - A record with OEM_REC_UNMAPPED takes no part: it cuts no cell and no read, and its barcode and name are never
 *     looked at (they may be empty or hold a 0 byte).  The other records are the survivors.
 *   - The survivors' barcodes and names are not empty and hold no 0 byte.
 *   - A cell is a maximal run of byte-equal barcodes among the survivors; a barcode that comes back later is a NEW cell
 *     with the same label (the reference has no memory of earlier barcodes either); cells are numbered in closing
 *     order, which is input order; there is no case folding.  Unlike the reference, an unmapped record that leads a
 *     run under a foreign barcode gives no empty cell (single_cell.rs:200-213 reads CB before it skips).
 *   - Inside a cell the name rule as it stands: OEM_COLLATE_SORT orders by name bytes, primary first, index;
 *     OEM_COLLATE_ADJACENT only cuts.  The same name in two cells is two reads.
 *   - The open cell -- the trailing run of one barcode so far -- is carried on the device from batch to batch; a batch's
 *     first run joins it when the barcodes are equal byte for byte; a batch closes every run but its last; a batch
 *     without a survivor changes nothing; finish closes the open cell.
 * With S the survivors' indices, ascending, oem_cells_stream_finish gives what oem_em_run_cells_records_names_sparse
 * gives on records[S], names[S], secondary[S] and the cell_rec_off of the rule, with the session's filters, model and
 * mode -- however the input was cut and whichever thread pushed what: cell_rec_off, order (S[order of the one call]),
 * group_off, cell_group_off, kept, the discard tables, the entries' offsets and columns and the cells' labels exactly,
 * values and infos as a session is held to its one call (which group a cell lands in may change the tile layout,
 * never the problem).  Cell k of the result is the k-th cell closed; tickets number batches, not cells.
 *
 * oem_cells_stream_push_barcodes, one batch: n_records records with one barcode and one name each (a blob and
 * n_records + 1 offsets from 0, as oem_collate_barcodes and oem_collate_names take them) and their secondary flags
 * (NULL: none is set).  Thread-safe.  Checked on the calling thread before the session is touched: both offset tables
 * present, starting at 0 and not decreasing; a blob present when its last offset is above 0; records present when
 * n_records > 0; n_records <= 2^31 - 2.  An argument error (OEM_ERR_ARG) rejects that batch only and uses no ticket.
 * Everything is copied into page-locked staging by the caller's thread: the arrays may be freed on return.  The call
 * blocks while more than max_staged_nnz RECORDS are staged and not yet on the device (a batch larger than that is
 * accepted when nothing else is staged).  An empty batch, and a batch of unmapped records only, takes a ticket and
 * changes nothing.  A parse worker takes the batches in ticket order: survivors, checks, the barcode cut, and the
 * survivors' records, names, flags and indices appended to a device arena of cells not yet run.  Once the arena's
 * closed cells reach group_nnz records or group_cells cells (the limits of oem_em_run_cells' own group rule always
 * apply) they run on the session's group workers -- collation, gather, filter, coverage model, EM -- while later
 * batches arrive; OEM_CELLS_STREAM_INFO_GROUPS_BEFORE_FINISH counts such groups, OEM_CELLS_STREAM_INFO_CELLS the
 * batches and OEM_CELLS_STREAM_INFO_ALIGNMENTS the records accepted.  Nothing run-sized exists on the host before
 * finish, and no cell is collated or gathered there; a group whose filter must take the host loop (no gap table for
 * score_prob_denom, a score beyond +-2^24) takes it, with the same result.
 *
 * Found on the device and sticky (every later push and finish returns the status and the message of the first):
 *   - an empty barcode or name, or one with a 0 byte, of a survivor: OEM_ERR_ARG, "record <i> has an empty barcode" /
 *     "the name of record <i> contains a 0 byte" as the one calls say it, with the batch's "ticket <t>" and the
 *     session-global index i;
 *   - a ref_id that is not below n_txps: OEM_ERR_ARG, naming "ticket <t>" and the session-global index;
 *   - a cell of more than 2^31 - 2 records: OEM_ERR_ARG;
 *   - an alignment outside its transcript under a coverage model: OEM_ERR_STATE, naming the cell;
 *   - running out of memory: OEM_ERR_OOM, with everything released.
 * On a barcoded session oem_cells_stream_push and oem_cells_stream_push_records return OEM_ERR_STATE; on the other
 * sessions the four calls below do. */
int oem_cells_stream_set_barcodes(oem_cells_stream *s, uint32_t mode /* OEM_COLLATE_SORT, OEM_COLLATE_ADJACENT */);
int oem_cells_stream_push_barcodes(oem_cells_stream *s, const oem_aln_record *records, uint64_t n_records,
                                   const uint8_t *barcodes, const uint64_t *barcode_off,
                                   const uint8_t *names, const uint64_t *name_off,
                                   const uint8_t *secondary /* or NULL */, uint64_t *out_ticket);
/* The ANY-ORDER form of the barcoded session: oem_em_run_cells_records_barcodes_sparse for a caller that never holds
 * the whole input -- a coordinate-sorted single-cell BAM read buffer by buffer, which the collated session above cannot
 * take.  Same preconditions and errors as oem_cells_stream_set_barcodes (a fresh records session only; a mode that is
 * neither value: OEM_ERR_ARG; on a plain session, after a push, after finish, or after either set_barcodes call:
 * OEM_ERR_STATE -- and oem_cells_stream_set_barcodes on such a session returns OEM_ERR_STATE too).  Batches arrive
 * through oem_cells_stream_push_barcodes, results leave through oem_cells_stream_finish, _barcodes_dims and
 * _barcodes_copy, all unchanged.
 *
 * The rule (oarfish_amd/csrc/oem_collate.h, "Cells from a stream in any order"): unmapped records take no part and
 * their bytes are never examined; a survivor's barcode and name are not empty and hold no 0 byte; a cell is the set of
 * survivors with one barcode, compared as bytes; cells are numbered by their first survivor, and a barcode that comes
 * back is the SAME cell; inside a cell the survivors keep session order and the name rule (mode) is then applied.
 * With S the survivors' indices, ascending, finish gives exactly what oem_em_run_cells_records_barcodes_sparse gives on
 * records[S], barcodes[S], names[S], secondary[S], however the input was cut and whichever thread pushed what:
 * cell_rec_off, group_off, cell_group_off, kept, the discard tables, the entries' offsets and columns, the labels in
 * cell order, and order as S[order of the one call]; values and infos as a session is held to its one call.
 *
 * Per batch the survivors' barcodes are interned on the device against a hash table of the labels seen so far, and
 * the arena keeps a 4-byte cell id per survivor instead of its barcode.  NOTHING RUNS BEFORE finish, because any
 * barcode may return: finish finds the cells with one stable integer sort of the cell ids, lays the arena out by cell
 * and runs the cells in groups as the collated session does (OEM_CELLS_STREAM_INFO_GROUPS_BEFORE_FINISH stays 0).
 * The arena therefore holds every survivor until finish: its records, names, flags, 64-bit indices and cell ids
 * (OEM_CELLS_STREAM_INFO_ARENA_BYTES).  Device-found errors are sticky, worded as the collated session's with "ticket
 * <t>" and the session-global index: a bad barcode or name; a ref_id not below n_txps, checked per batch; more than
 * 2^31 - 2 survivors in the session, refused at the batch that crosses (OEM_ERR_ARG); OEM_ERR_OOM with everything
 * released. */
int oem_cells_stream_set_barcodes_any_order(oem_cells_stream *s, uint32_t mode /* OEM_COLLATE_SORT, OEM_COLLATE_ADJACENT */);
/* A UMI SESSION: oem_em_run_cells_records_umis_sparse's deduplication for the two barcoded sessions, so that a reader
 * of a single-cell BAM need not deduplicate first (the reference wants "already (UMI) deduplicated reads",
 * docs/index.md:308-312).  oem_cells_stream_set_umis comes after either set_barcodes call and before any push.  On a
 * session that is not barcoded, after a push, after finish, or a second time: OEM_ERR_STATE.  On a UMI session
 * oem_cells_stream_push_barcodes returns OEM_ERR_STATE; on every other session oem_cells_stream_push_barcodes_umis does.
 *
 * The rule (oarfish_amd/csrc/oem_collate.h, "UMIs in the sessions").  Every batch carries one UMI byte string per
 * record (umis with n_records + 1 offsets from 0); the empty string means no UB tag.  An unmapped record's UMI is never
 * examined; a survivor's UMI may be empty and may not hold a 0 byte.  Cells are cut or interned by the form's own rule;
 * inside a cell, behind the name collation, the reads whose heads carry the same non-empty UMI are one class, its
 * smallest read survives and the others leave with all their records (oem_dedup_umis' rule).  Classes never span
 * cells.  With S the survivors' indices, ascending:
 *   - any-order form: finish gives exactly what oem_em_run_cells_records_umis_sparse gives on records[S], barcodes[S],
 *     names[S], secondary[S], umis[S], order being S[order of the one call];
 *   - collated form (a barcode that comes back is a NEW cell, so no one call names it): oem_collate_names on the
 *     S-arrays with the streamed rule's cell_rec_off, oem_dedup_umis on its output with umis[S], the duplicates'
 *     positions dropped, oem_em_run_cells_records_sparse on what remains.  Two runs of one barcode that hold the same
 *     UMI keep both reads.
 * A session all of whose UMIs are empty gives exactly the result of the same session without UMIs.
 *
 * oem_cells_stream_push_barcodes_umis has oem_cells_stream_push_barcodes' preconditions and checks on the calling
 * thread: umi_off present, from 0 and not decreasing; umis present when its last offset is above 0.  An argument error
 * rejects that batch only and uses no ticket.  The UMIs are copied into page-locked staging with the rest; no UMI byte
 * is touched by the host between staging and the result.  A survivor's UMI with a 0 byte is found on the device and is
 * sticky: OEM_ERR_ARG, "the UMI of record <i> contains a 0 byte" with the batch's "ticket <t>" and the session-global
 * index; the smallest such index of the batch wins, and on one record the order is barcode, name, UMI.
 *
 * A bad ref_id: the sessions differ from the one call and from each other.  The any-order form checks ref_id per batch
 * on every surviving record, so a bad ref_id in a record that would later turn out to be a duplicate is an error there;
 * the collated form finds it in the group, among the reads that remain.  The any-order form's bound of 2^31 - 2
 * survivors counts the duplicates' records too.
 *
 * After finish, oem_cells_stream_barcodes_dims / _barcodes_copy describe the DEDUPLICATED collation: n_survivors counts
 * the positions of out_order and out_cell_rec_off counts positions of it, n_groups counts the reads that remain,
 * n_unmapped is unchanged; records accepted = n_unmapped + n_survivors + OEM_CELLS_STREAM_INFO_UMI_DUP_RECORDS.  A
 * duplicate is in no discard table.  oem_cells_stream_umis_copy gives the duplicates (reads) dropped from every cell
 * (n_cells entries); before finish, or on a session without UMIs: OEM_ERR_STATE.  The arena keeps a survivor's UMI and
 * an 8-byte offset beside its name (OEM_CELLS_STREAM_INFO_ARENA_BYTES counts them). */
int oem_cells_stream_set_umis(oem_cells_stream *s);
int oem_cells_stream_push_barcodes_umis(oem_cells_stream *s, const oem_aln_record *records, uint64_t n_records,
                                        const uint8_t *barcodes, const uint64_t *barcode_off,
                                        const uint8_t *names, const uint64_t *name_off,
                                        const uint8_t *secondary /* or NULL */,
                                        const uint8_t *umis, const uint64_t *umi_off, uint64_t *out_ticket);
int oem_cells_stream_umis_copy(const oem_cells_stream *s, uint64_t *out_cell_dups /* n_cells */);
/* THE UMI RULE IN A UMI SESSION: oem_cells_stream_set_umi_rule gives a UMI session of either form the oem_umi_rule of
 * oem_em_run_cells_records_umis_rule_sparse -- gene-aware keys (gene_of, one gene id per transcript) and one-mismatch
 * correction (correct) -- in every group's deduplication.  It is called after oem_cells_stream_set_umis, before the first
 * push, and once: anything else is OEM_ERR_STATE.  OEM_ERR_ARG: rule NULL; correct > 1; gene_of given with n_txps == 0
 * or with an n_txps that is not the session's.  gene_of is copied.  {NULL, 0, 0} is accepted and is the exact rule: the
 * session then gives what it gives without this call.  The genes come from the records' own ref_id words, at the heads
 * of the reads that take part.  With S the survivors' indices, ascending:
 *   - any-order form: finish gives exactly what oem_em_run_cells_records_umis_rule_sparse gives on the S-arrays under
 *     the same rule (correction reaches every record of a barcode, wherever it was pushed);
 *   - collated form: the join of oem_cells_stream_set_umis' description with oem_dedup_umis_rule (ref_id = the ref_ids
 *     of records[S]) in place of oem_dedup_umis.  A barcode that comes back is a new cell: nothing is corrected across
 *     the two.
 * A bad ref_id: the any-order form rejects the record's batch as before.  In the collated form the rule may meet a head
 * of a read that takes part before the filter does; the sticky error is the filter's own,
 * "ticket <t>: record <i>: ref_id <x> is not below n_txps", with the session-global index.
 * After a successful finish of a session whose rule has correct, oem_cells_stream_umi_rule_copy gives the reads corrected
 * in every cell (n_cells entries, in cell order), as out_cell_corrected of the one call; otherwise OEM_ERR_STATE.
 * OEM_CELLS_STREAM_INFO_UMI_CORRECTED_READS is their sum over the groups that have run. */
int oem_cells_stream_set_umi_rule(oem_cells_stream *s, const oem_umi_rule *rule);
int oem_cells_stream_umi_rule_copy(const oem_cells_stream *s, uint64_t *out_cell_corrected /* n_cells */);
/* THE BARCODE RULE IN THE ANY-ORDER SESSION: oem_cells_stream_set_whitelist gives an any-order barcoded session the
 * oem_barcode_rule of oem_em_run_cells_records_whitelist_sparse.  The batches' barcodes are then RAW (CR tags): every batch
 * is matched against the whitelist on the device, and the session's cells are the whitelist's labels.  It is called after
 * oem_cells_stream_set_barcodes_any_order and before the first push, once, in either order with oem_cells_stream_set_umis
 * / _set_umi_rule; the rule's arrays are copied.  OEM_ERR_ARG: the rule's own checks, a whitelist of 2^31 labels or more,
 * and the whitelist errors found on the device (a label with a 0 byte, two equal labels), worded as oem_correct_barcodes
 * words them.  OEM_ERR_STATE: on a plain or records session, after a push, after finish, a second time -- and on the
 * COLLATED barcoded session, on purpose: its cells are runs of byte-equal barcodes and a barcode that comes back is a new
 * cell, so corrected raw barcodes would scatter one label over many cells; use the any-order form.
 *
 * The rule in a session.  n(w) grows batch by batch, so a batch decides what does not depend on it and defers the rest:
 *   - an unmapped record takes no part: its barcode is never examined and it adds nothing to n(w) (oem_correct_barcodes
 *     and the one call count it: on input that holds unmapped records they differ from the session, which equals them on
 *     the mapped records' arrays);
 *   - a mapped record's barcode may be empty (OEM_BARCODE_MISSING); a 0 byte in it is the batch's sticky OEM_ERR_ARG,
 *     naming ticket and session-global index;
 *   - exact records get their label and raise n(w); a miss with no neighbour, with one neighbour, or -- multi = 0 -- with
 *     several is decided in its batch; only multi = 1 with several neighbours is DEFERRED to finish, which decides it with
 *     the complete counts;
 *   - a record rejected in its batch is dropped there: its name, UMI and ref_id are NEVER LOOKED AT, as the one call
 *     promises.  The name and UMI checks and the batch's ref_id check run over the retained records -- the accepted and the
 *     deferred ones.  THE SESSIONS DIFFER in this: a deferred record is checked in its batch, so an error in it is an
 *     error of the session even if finish then rejects it; the one call never sees that error;
 *   - cells are numbered by their first accepted record in session order -- which may be a deferred one: the numbering is
 *     made at finish, not by first sight -- with session order inside a cell; a cell's label is the whitelist's bytes.
 * With S the mapped records' indices, ascending, finish gives exactly what oem_em_run_cells_records_whitelist_sparse
 * gives on records[S], barcodes[S], names[S], secondary[S], umis[S] under the same rules, however the input is cut and
 * whichever thread pushes what: order is S[order of the one call]; values and infos as a session is held to its one call.
 * The bound of 2^31 - 2 records counts the retained records.  Batches arrive through oem_cells_stream_push_barcodes /
 * _push_barcodes_umis, unchanged.  After finish, oem_cells_stream_barcodes_dims / _barcodes_copy describe the ACCEPTED
 * records: records pushed = n_unmapped + OEM_CELLS_STREAM_INFO_BARCODE_REJECTED + positions of order +
 * OEM_CELLS_STREAM_INFO_UMI_DUP_RECORDS.  oem_cells_stream_whitelist_copy gives, after a successful finish of a whitelist
 * session (otherwise OEM_ERR_STATE), every cell's label index, the number of its records that were corrected and the
 * records of each of the five statuses; each output may be NULL.  Resident beyond the any-order session: the whitelist
 * (as in oem_correct_barcodes) and the deferred records' barcodes with 4 bytes each, counted by
 * OEM_CELLS_STREAM_INFO_ARENA_BYTES. */
int oem_cells_stream_set_whitelist(oem_cells_stream *s, const oem_barcode_rule *rule);
int oem_cells_stream_whitelist_copy(const oem_cells_stream *s, uint32_t *out_cell_wl_id /* n_cells */,
                                    uint64_t *out_cell_bc_corrected /* n_cells */, uint64_t *out_counts /* 5 */);
/* After a successful oem_cells_stream_finish of a barcoded session (otherwise OEM_ERR_STATE): the sizes of what
 * oem_cells_stream_barcodes_copy gives (each may be NULL) -- the cells, the survivors, the reads (record groups) of all
 * cells, the bytes of all labels, and the unmapped records that were skipped. */
int oem_cells_stream_barcodes_dims(const oem_cells_stream *s, uint64_t *n_cells, uint64_t *n_survivors,
                                   uint64_t *n_groups, uint64_t *barcode_bytes, uint64_t *n_unmapped);
/* out_barcodes (barcode_bytes) with out_barcode_off (n_cells + 1): the cells' labels in cell order;
 * out_cell_rec_off (n_cells + 1): the cells' first positions among the survivors; out_order (n_survivors): the
 * session-global index of the record at every collated position; out_group_off (n_groups + 1): the positions where a
 * read starts, then n_survivors; out_cell_group_off (n_cells + 1); out_kept (n_groups): the alignments the filter kept
 * per read.  Each may be NULL; the two barcode outputs only together (OEM_ERR_ARG). */
int oem_cells_stream_barcodes_copy(const oem_cells_stream *s, uint8_t *out_barcodes, uint64_t *out_barcode_off,
                                   uint64_t *out_cell_rec_off, uint64_t *out_order, uint64_t *out_group_off,
                                   uint64_t *out_cell_group_off, uint32_t *out_kept);
/* Runs what is still staged, waits for every group and returns the cells in ticket order as an ordinary
 * oem_cells_result (oem_cells_result_dims / _copy / _destroy; infos included).  Per cell the result is what
 * oem_em_run_cells_sparse (coverage = 1: oem_em_run_cells_coverage_sparse) gives for that cell, up to floating-point
 * summation order: which group a cell lands in may change the tile layout, never the problem.  A session without
 * cells gives a result with 0 cells.  While a push is in flight, or a second time: OEM_ERR_STATE.  *out = NULL on any
 * failure. */
int oem_cells_stream_finish(oem_cells_stream *s, oem_cells_result **out);
int oem_cells_stream_info(const oem_cells_stream *s, uint32_t key, uint64_t *value);
/* NULL: no-op.  Before finish: cancels -- groups not yet started are dropped, a group on the device runs to its end,
 * the workers are joined.  No push may be in flight. */
void oem_cells_stream_destroy(oem_cells_stream *s);

/* A bulk RECORDS SESSION: oem_store_create_records for a caller that never holds all records at once (the reference's
 * parse_alignments, alignment_parser.rs:301-437, adds group by group; its raw-read drivers, bulk.rs:364-682, hand
 * chunks from mapper threads to a consumer).  Batches of whole groups are pushed from any number of threads as they are
 * parsed; each pushing thread copies its batch into page-locked staging, one device worker filters the batches in ticket
 * order while later ones arrive, a batch's records leave the device once its alignments are emitted, and finish joins
 * the batches' CSR pieces on the device into the store.  One device per session. */
typedef struct oem_records_stream oem_records_stream;

typedef struct {
    uint32_t n_txps;
    int32_t  device;
    uint32_t bin_width;          /* as oem_store_create_records */
    int32_t  model;              /* -1 no coverage column, 0 logistic, 1 binomial */
    double   growth_rate;
    uint64_t max_staged_records; /* 0 = default; push blocks while more than this is staged and not yet on the device */
    uint32_t reserved[4];        /* 0 */
} oem_records_stream_opts;

#define OEM_RECORDS_STREAM_INFO_BATCHES 1u               /* batches accepted */
#define OEM_RECORDS_STREAM_INFO_GROUPS 2u                /* groups accepted */
#define OEM_RECORDS_STREAM_INFO_RECORDS 3u               /* records accepted */
#define OEM_RECORDS_STREAM_INFO_BATCHES_BEFORE_FINISH 4u /* batches whose device pass had started before
                                                            oem_records_stream_finish was called */
#define OEM_RECORDS_STREAM_INFO_BLOCKED_US 5u            /* microseconds pushes spent blocked on back-pressure, summed
                                                            over the pushing threads */
#define OEM_RECORDS_STREAM_INFO_HOST_BATCHES 6u          /* batches the host loop took (a score beyond +-2^24, or a
                                                            score_prob_denom without a table) */
#define OEM_RECORDS_STREAM_INFO_ROW_NAME_BYTES 7u        /* a names session, after finish: bytes of the rows' names */

/* Argument errors (opts, filters, txp_len or out NULL, n_txps = 0, a model outside -1 .. 1, bin_width = 0 under a
 * model, a non-zero reserved word) are reported before any device is touched; without a device the call returns
 * OEM_ERR_NO_DEVICE.  filters and txp_len (n_txps entries) are copied.  *out = NULL on any failure. */
int oem_records_stream_create(const oem_records_stream_opts *opts, const oem_filters *filters, const uint64_t *txp_len,
                              oem_records_stream **out);
/* One batch of whole groups, as oem_store_create_records takes all of them (group_off: n_groups + 1 entries from 0).
 * Thread-safe.  Checked on the calling thread: group_off starts at 0 and does not decrease, no group has more than
 * 2^32 - 1 records, at most 2^31 - 2 groups; an argument error (OEM_ERR_ARG) rejects that batch only, uses no ticket and
 * leaves the session usable.  The arrays are copied into page-locked staging by the calling thread: the caller may free
 * them on return.  *out_ticket (optional) receives the batch's ticket: 0, 1, 2 ... in the order in which pushes were
 * accepted; the session's input is the batches in ticket order.  A batch without groups is accepted and takes a ticket.
 * The call blocks while more than max_staged_records records are staged and not yet on the device, except that a batch
 * larger than that budget is accepted when nothing else is staged.  A ref_id that is not below n_txps is found on the
 * device: it is sticky and its message names the batch ("ticket <ticket>") and the record's index within the batch.
 * Device and allocation failures are sticky too: every later push and finish returns that status and its message.
 * 2^32 or more kept alignments in all: OEM_ERR_ARG, sticky.  After finish: OEM_ERR_STATE. */
int oem_records_stream_push(oem_records_stream *s, const oem_aln_record *records, const uint64_t *group_off,
                            uint64_t n_groups, uint64_t *out_ticket);
/* Waits for the batches still staged, joins the pieces and returns what oem_store_create_records returns for the
 * concatenation of the accepted batches in ticket order, with the session's filters, txp_len, bin_width, model and
 * growth_rate and these opts: the same store (row r is the r-th group, in ticket order, with out_kept > 0), out_kept
 * (one entry per accepted group) and out_discard, however the input was cut into batches and whichever thread pushed
 * what.  A session without batches gives a store of 0 reads.  opts are checked first (OEM_ERR_ARG leaves the session as
 * it was).  While a push is in flight, or a second time: OEM_ERR_STATE.  *out = NULL on any failure. */
int oem_records_stream_finish(oem_records_stream *s, const oem_store_opts *opts,
                              uint32_t *out_kept /* all groups, ticket order; or NULL */,
                              oem_discard_table *out_discard /* or NULL */, oem_store **out);
int oem_records_stream_info(const oem_records_stream *s, uint32_t key, uint64_t *value);
/* NULL: no-op.  Before finish: cancels -- batches not yet started are dropped, the batch on the device runs to its end,
 * the worker is joined.  No push may be in flight. */
void oem_records_stream_destroy(oem_records_stream *s);

/* The NAMES form of the session: oem_store_create_records_names for a caller that never holds all records or names at
 * once (parse_alignments walks a BAM reader record by record).  Batches are records and their read names in input
 * order, cut at ANY record positions -- a read may straddle two batches, or any number of them.
 *
 * The contract.  Let R, names, name_off be the accepted batches concatenated in ticket order.  finish_names gives
 * exactly what oem_store_create_records_names(filters, txp_len, n_txps, R, names, name_off, secondary = NULL,
 * OEM_COLLATE_ADJACENT, sort_check_num, ...) gives with the session's filters, txp_len, bin_width, model and
 * growth_rate and finish's opts, however the input was cut into batches, cuts inside a read included: the store (CSR
 * and weights bit for bit), out_group_off, out_kept, the discard table, every field of oem_parse_info, the row names and
 * their offsets.  out_order has no session form: under OEM_COLLATE_ADJACENT it is the ascending input indices of the
 * records without OEM_REC_UNMAPPED, which the caller already has.  How a batch's surviving records attach to the open
 * read is stated once, in oarfish_amd/csrc/oem_collate.h (ParseBulkStream): the open read -- the trailing run of one
 * name among the survivors so far -- is carried on the device from batch to batch; a batch's first run joins it when
 * the names are equal byte for byte; a batch closes every run but its last; a batch without a survivor changes nothing;
 * finish closes the open read.  A record's index in messages is session-global: it counts all records of all accepted
 * batches in ticket order, unmapped ones included, in 64 bits.
 *
 * oem_records_stream_set_names turns a fresh session into a names session (oem_records_stream_opts has no room for the
 * parameter: its reserved words stay 0).  After a push, after finish, or a second time: OEM_ERR_STATE.  On a names
 * session oem_records_stream_push and oem_records_stream_finish return OEM_ERR_STATE; on a plain one
 * oem_records_stream_push_names and oem_records_stream_finish_names do. */
int oem_records_stream_set_names(oem_records_stream *s, uint64_t sort_check_num);
/* One batch: records (n_records) with names / name_off as oem_store_create_records_names takes them for the whole
 * input.  There is no `secondary` argument: only OEM_COLLATE_SORT reads it, and a session cannot sort what it has not
 * seen (the sorting names form, oem_records_stream_set_sort below, holds the survivors until finish for that).
 * Thread-safe; tickets, back-pressure (max_staged_records, counted in records) and the reuse of staging memory
 * are oem_records_stream_push's.  Checked on the calling thread before the session is touched: name_off present,
 * starting at 0 and not decreasing; names present when name_off[n_records] > 0; records present when n_records > 0;
 * n_records <= 2^31 - 2.  An argument error (OEM_ERR_ARG) rejects that batch only and uses no ticket.  Records, offsets
 * and name bytes are copied into page-locked staging by the calling thread: the caller may free its arrays on return.
 * An empty batch, and a batch of unmapped records only, is accepted, takes a ticket and changes nothing else.
 *
 * Found on the device, sticky (every later push and finish returns the status and message), the first batch in ticket
 * order that has a fault reporting it: a surviving record with an empty name or a 0 byte in its name (OEM_ERR_ARG,
 * naming the record by its session-global index); a ref_id that is not below n_txps (OEM_ERR_ARG, naming "ticket
 * <ticket>" and the session-global index); 2^32 or more kept alignments (OEM_ERR_ARG); a read of more than 2^32 - 1
 * records (OEM_ERR_ARG).  The collation check covers the first min(sort_check_num, n_groups) groups of the SESSION: the
 * head names of the closed groups are held on the device until sort_check_num of them are there, or until finish; the
 * one call's check runs once then.  A repeat is OEM_ERR_STATE with the one call's message on the concatenation (the
 * same group, first-record index and earlier index); being sticky it may surface at the push after the one that closed
 * group sort_check_num - 1, or at finish.  A repeat at a group index >= sort_check_num is accepted.  The host loop takes
 * a batch's closed groups where oem_records_stream_push's would (OEM_RECORDS_STREAM_INFO_HOST_BATCHES counts them). */
int oem_records_stream_push_names(oem_records_stream *s, const oem_aln_record *records, uint64_t n_records,
                                  const uint8_t *names, const uint64_t *name_off, uint64_t *out_ticket);
/* Waits for the staged batches, closes the open read, runs the collation check if it is still pending, joins the pieces
 * on the device and returns the store of the contract above, with the discard table and the parse info.  An alignment
 * outside its transcript under a coverage model: OEM_ERR_STATE.  The variable-length outputs stay with the session
 * (oem_records_stream_names_copy).  A session without a surviving record gives the store of no groups.  opts are
 * checked first (OEM_ERR_ARG leaves the session as it was).  While a push is in flight, or a second time:
 * OEM_ERR_STATE.  *out = NULL on any failure. */
int oem_records_stream_finish_names(oem_records_stream *s, const oem_store_opts *opts,
                                    oem_discard_table *out_discard /* or NULL */, oem_parse_info *out_info /* or NULL */,
                                    oem_store **out);
/* After a successful oem_records_stream_finish_names (before: OEM_ERR_STATE): out_group_off (n_groups + 1 positions
 * among the surviving records), out_kept (n_groups), out_row_names (OEM_RECORDS_STREAM_INFO_ROW_NAME_BYTES bytes) and
 * out_row_name_off (n_reads + 1 offsets from 0).  Each may be NULL, the two row-name outputs only together. */
int oem_records_stream_names_copy(const oem_records_stream *s, uint64_t *out_group_off, uint32_t *out_kept,
                                  uint8_t *out_row_names, uint64_t *out_row_name_off);

/* The PROJECTED form of the session: oem_store_create_projected_records for a genome-mode caller that projects and
 * filters reads as they come (parse_genome_alignments, alignment_parser.rs:580-700, adds read by read; the mapper threads
 * of quantify_genome_raw_reads, bulk.rs:337-682, hand chunks to a consumer) and never holds a run-sized oem_proj_record
 * array.  Batches are whole groups, as oem_records_stream_push takes them, with one read length per group.
 *
 * oem_records_stream_set_projected turns a fresh session into a projected session, as oem_records_stream_set_names
 * turns one into a names session (oem_records_stream_opts has no room for the parameter).  popts is copied.  NULL
 * session, NULL popts or a prob_source outside 0 .. 2: OEM_ERR_ARG.  After a push, after finish, a second time or on a
 * names session: OEM_ERR_STATE; oem_records_stream_set_names on a projected session is OEM_ERR_STATE too.  On a
 * projected session oem_records_stream_push, _push_names, _finish_names and _names_copy return OEM_ERR_STATE; on a plain
 * or names session oem_records_stream_push_projected does. */
int oem_records_stream_set_projected(oem_records_stream *s, const oem_proj_opts *popts);
/* One batch of whole groups: records / group_off (n_groups + 1 entries from 0) / read_len (n_groups entries) as
 * oem_store_create_projected_records takes them for the whole input.  Thread-safe; tickets, back-pressure and the reuse
 * of staging memory are oem_records_stream_push's.  Checked on the calling thread before the session is looked at:
 * group_off present, starting at 0 and not decreasing, no group of more than 2^32 - 1 records, records present when
 * there are any, read_len present when there are groups, at most 2^31 - 2 groups.  An argument error (OEM_ERR_ARG)
 * rejects that batch only, uses no ticket and leaves *out_ticket untouched.  The three arrays are copied into page-locked
 * staging by the calling thread.
 *
 * The device worker runs the pass of oem_builder_add_projected_groups_device on each batch.  Under OEM_PROJ_SIMILARITY
 * and _COMBINED the alignments whose device exponential is not provably libm's are not finished batch by batch: each
 * batch keeps their (index, f) pairs on the device, finish joins the lists and the host applies expf once
 * (OEM_RECORDS_STREAM_INFO_HOST_FINISHED).  The host loop takes a batch with |aln_score| > 2^24, and every batch when
 * score_prob_denom has no table under OEM_PROJ_SCORE or beta is not finite under the other two sources
 * (OEM_RECORDS_STREAM_INFO_HOST_BATCHES).  A ref_id that is not below n_txps, or that names a transcript of length 0, is
 * found on the device: OEM_ERR_ARG, sticky, its message naming "ticket <ticket>", the record's index within the batch
 * and the ref_id.
 *
 * oem_records_stream_finish on a projected session returns what oem_store_create_projected_records returns for the
 * accepted batches concatenated in ticket order, with the session's filters, txp_len, popts, bin_width, model and
 * growth_rate and finish's opts: the same store (row pointers, ids and as_prob bit for bit, the same coverage column),
 * out_kept and out_discard, however the input was cut into batches. */
int oem_records_stream_push_projected(oem_records_stream *s, const oem_proj_record *records,
                                      const uint64_t *group_off, const uint64_t *read_len,
                                      uint64_t n_groups, uint64_t *out_ticket);
#define OEM_RECORDS_STREAM_INFO_HOST_FINISHED 8u /* a projected session, after finish: alignments whose expf the host
                                                    supplied; 0 on a plain or names session */

/* The SORTING NAMES form of the session: oem_store_create_records_names under OEM_COLLATE_SORT for a caller that never
 * holds all records or names at once -- a coordinate-sorted or unsorted BAM read batch by batch.  Batches are records,
 * their read names and (optionally) their secondary flags, in any order and cut at any record positions: the records
 * of one read may lie in any number of batches, a secondary before its primary.
 *
 * The contract.  Let R, names, name_off, secondary be the accepted batches concatenated in ticket order (a batch
 * pushed without flags counting as flags of 0).  finish_names gives exactly what oem_store_create_records_names(...,
 * R, names, name_off, secondary, OEM_COLLATE_SORT, sort_check_num = 0, ...) gives for them with the session's filters,
 * txp_len, bin_width, model and growth_rate and finish's opts, wherever the batches were cut: the store (CSR and
 * weights bit for bit, for every weight_coding and layout_build), out_group_off, out_kept, the discard table, the row
 * names and their offsets, every field of oem_parse_info (n_checked = 0), and out_order -- as 64-bit session-global
 * input indices (oem_records_stream_order_copy), which count all records of all accepted batches in ticket order,
 * unmapped ones included.  The rule is stated once, in oarfish_amd/csrc/oem_collate.h (ParseBulkSortStream).
 *
 * A session cannot sort what it has not seen: nothing is cut or filtered before finish.  The device worker uploads
 * each batch, drops its unmapped records, checks and densifies the survivors' names and appends the survivors -- 40
 * bytes of record, the name, one flag byte, 8 bytes of offset and 8 of index each -- to an arena that stays on the
 * device and grows by doubling (OEM_RECORDS_STREAM_INFO_ARENA_BYTES); finish collates the arena as one batch and goes
 * on as the one call does.  Device memory is therefore the one call's, not less: what the session saves is the
 * run-sized host arrays.
 *
 * oem_records_stream_set_sort turns a fresh session into a sorting names session.  After a push, after another
 * oem_records_stream_set_*, after finish, or a second time: OEM_ERR_STATE.  On a sorting names session
 * oem_records_stream_push, _push_names, _push_projected and _finish return OEM_ERR_STATE; on any other session
 * oem_records_stream_push_sort and oem_records_stream_order_copy do.  oem_records_stream_finish_names and
 * oem_records_stream_names_copy serve it as they serve a names session. */
int oem_records_stream_set_sort(oem_records_stream *s);
/* One batch: as oem_records_stream_push_names, with `secondary` (n_records flags, or NULL for none) besides.  The
 * argument checks, made on the calling thread before the session is touched, and staging, tickets and back-pressure
 * are oem_records_stream_push_names'; a rejected batch uses no ticket.
 *
 * Found on the device, sticky as in a names session, the first batch in ticket order that has a fault reporting it: a
 * surviving record with an empty name or a 0 byte in its name (OEM_ERR_ARG, naming the record's session-global index);
 * a surviving record's ref_id that is not below n_txps (OEM_ERR_ARG, naming "ticket <ticket>" and the session-global
 * index); more than 2^31 - 2 surviving records in the session (OEM_ERR_ARG at the batch that crosses: the collation is
 * one batch); out of device memory (OEM_ERR_OOM).  After a sticky error the arena is released.  Where the host loop
 * takes the groups (a score beyond +-2^24, or a score_prob_denom without a table) the survivors come down from the
 * arena once, at finish, and OEM_RECORDS_STREAM_INFO_HOST_BATCHES is 1. */
int oem_records_stream_push_sort(oem_records_stream *s, const oem_aln_record *records, uint64_t n_records,
                                 const uint8_t *names, const uint64_t *name_off, const uint8_t *secondary /* or NULL */,
                                 uint64_t *out_ticket);
/* After a successful oem_records_stream_finish_names on a sorting names session (before, or on another session:
 * OEM_ERR_STATE): out_order, n_parsed session-global input indices -- the surviving records collated by the name rule,
 * what oem_store_create_records_names writes to its out_order in 32 bits. */
int oem_records_stream_order_copy(const oem_records_stream *s, uint64_t *out_order);
#define OEM_RECORDS_STREAM_INFO_ARENA_BYTES 9u /* a sorting names session: the most device bytes its arena has held
                                                  (a growing array counted twice while it is copied); 0 otherwise */

/* --------------------------------------------------------------------- */
/* multi-GPU (row shards + one RCCL all-reduce of the count vector / pass) */
/* --------------------------------------------------------------------- */

#define OEM_UNIQUE_ID_BYTES 128
/* Rank 0 obtains an id and hands it to the other ranks through whatever the
 * host uses (torch.distributed broadcast, MPI, a file ...). */
int oem_comm_unique_id(void *out_id /* OEM_UNIQUE_ID_BYTES */);
int oem_comm_create(const void *unique_id, int rank, int n_ranks, int device, oem_comm **out);
void oem_comm_destroy(oem_comm *comm);

/* The one-shot peer-to-peer exchange (oem_p2p.hip): every rank publishes its partial count vector in a
 * buffer its peers have mapped (hipIpc memory handles between processes; plain pointers between ranks
 * that are threads of one process) and sums the N partials itself, in rank order -- bit-identical on
 * every rank, no ring, no RCCL.  It serves vectors of up to 4 MB (the 1.6 MB count vector of a
 * 200 k-transcript store is latency-bound; the reference's analogue is the shared Vec<AtomicF64> of
 * em.rs:338-341); larger exchanges stay with RCCL when the communicator has one.
 *   oem_comm_create(NULL, rank, n_ranks > 1, ...) makes a communicator without RCCL;
 *   oem_comm_p2p_export: allocates this rank's exchange buffer for vectors of up to `capacity` doubles
 *     (n_txps, or n_txps * 4 to cover the batched bootstrap of a row-sharded store) and writes its
 *     handle (OEM_P2P_HANDLE_BYTES bytes), which the host gathers over whatever it has (as the unique id);
 *   oem_comm_p2p_connect: `all_handles` = the n_ranks handles in rank order; maps the peers' buffers.
 * All ranks must export the same capacity.  Needs HSA_ENABLE_IPC_MODE_LEGACY=0 where the driver only
 * supports dmabuf IPC.  A rank that waits more than 8 s for a peer fails with OEM_ERR_STATE. */
#define OEM_P2P_HANDLE_BYTES 128
int oem_comm_p2p_export(oem_comm *comm, uint64_t capacity, void *out_handle /* OEM_P2P_HANDLE_BYTES */);
int oem_comm_p2p_connect(oem_comm *comm, const void *all_handles /* n_ranks x OEM_P2P_HANDLE_BYTES */);

/* Collective (every rank, same value).  OEM_COMM_OPT_P2P_MAX_BYTES: largest vector, in bytes, that takes
 * the peer-to-peer exchange when the communicator also has RCCL (default 4 MB; 0 = always RCCL).
 * OEM_COMM_OPT_P2P_SHAPE: 0 (default) = by the number of ranks and the vector's size, 1 = one-shot (every rank reads every
 * partial whole), 2 = two-phase (rank r sums slice r, then every rank reads the reduced slices from their
 * owners: a quarter of the bytes per xGMI link at 8 ranks for one more flag round); oem_p2p.hip.
 * OEM_COMM_OPT_P2P_TIMEOUT_MS: bound of one wait for a peer inside an exchange kernel, in milliseconds (default
 * 8000; a wait that gives up ends the run with OEM_ERR_STATE instead of hanging the GPU).
 * OEM_COMM_OPT_P2P_SELF_CHECK (set BEFORE oem_comm_p2p_connect): 1 = connect ends with a checked exchange in both
 * shapes against a closed-form sum -- also the ranks' rendezvous, with a long wait (120 s), so a peer that is still
 * building its store does not time the EM loop's first exchange out.  Needs every rank inside connect at the same
 * time (ranks = processes); a failure leaves the peer-to-peer backend disconnected (RCCL, if any, carries on).
 * Value 2, AFTER oem_comm_p2p_connect: run that checked exchange now -- for hosts that first make sure every rank has
 * mapped its peers (oarfish_amd.dist gathers one byte per rank), so that a rank whose connect failed does not leave the
 * others waiting in a kernel for the rendezvous bound (the longer of OEM_COMM_OPT_P2P_TIMEOUT_MS and 120 s). */
typedef enum { OEM_COMM_OPT_P2P_MAX_BYTES = 1, OEM_COMM_OPT_P2P_SHAPE = 2, OEM_COMM_OPT_P2P_TIMEOUT_MS = 3,
               OEM_COMM_OPT_P2P_SELF_CHECK = 4 } oem_comm_option;
int oem_comm_set_option(oem_comm *comm, uint32_t option, uint64_t value);

/* What a communicator is made of, for the host's records (bench.py's config.exchange): OEM_COMM_INFO_RANKS = n_ranks
 * as created; OEM_COMM_INFO_RCCL_RANKS = the number of ranks RCCL itself reports for its communicator
 * (ncclCommCount; 0 without RCCL) -- the first multi-GPU run says from the library's own mouth how many ranks the
 * collective spanned; OEM_COMM_INFO_P2P_CONNECTED = 1 when the peer-to-peer exchange is mapped on this rank. */
typedef enum { OEM_COMM_INFO_RANKS = 1, OEM_COMM_INFO_RCCL_RANKS = 2, OEM_COMM_INFO_P2P_CONNECTED = 3 } oem_comm_info_key;
int oem_comm_info(const oem_comm *comm, uint32_t key, uint64_t *out);

/* Declare `store` to be rank-local row shard of a store with
 * `global_n_reads` reads in total (needed for the uniform init, em.rs:154,165).
 * After this, oem_em_run / oem_bootstrap on the shard are collective calls:
 * every rank must make them with the same arguments; each pass all-reduces
 * (sum, f64) the n_txps partial counts over `comm`, after which all ranks take
 * the identical convergence decision. */
int oem_store_attach_comm(oem_store *store, oem_comm *comm, uint64_t global_n_reads,
                          uint64_t global_row_offset);

/* --------------------------------------------------------------------- */
/* measurement                                                            */
/* --------------------------------------------------------------------- */

/* Launch the E/M kernel `n_launches` times back to back on the store's
 * stream, bracketed by HIP events on that stream; returns the average
 * launch duration in milliseconds (bench.py's roofline.achieved). */
int oem_time_m_step(oem_store *store, uint32_t n_launches, float *out_avg_ms);

/* Run exactly `n_iters` loop iterations (E/M pass + rel-diff + swap/clear,
 * em.rs:181-207) from the uniform init with no convergence exit, timed with
 * HIP events on the store's stream; out_ms = total milliseconds. */
int oem_time_em_iters(oem_store *store, uint32_t n_iters, float *out_ms);

/* Run `n_passes` batched bootstrap passes (tile + fold + rel-diff kernels of oem_bootstrap's
 * rolling batch) with every slot running its own device-drawn resample and no slot ever stopping,
 * timed with HIP events on the store's stream.  out_avg_ms = milliseconds per batched pass;
 * out_slots = replicates served by one pass; out_algorithmic_bytes = SURVEY.md section 8d's bytes
 * of one batched pass (matrix once, row weights + theta/counts per replicate).  OEM_ERR_STATE when
 * the store runs its bootstraps one per pass (wide windows, no tiled layout). */
int oem_time_bootstrap_passes(oem_store *store, uint32_t n_passes, float *out_avg_ms, uint32_t *out_slots,
                              uint64_t *out_algorithmic_bytes);

/* Collective on a store with an attached communicator: `n_calls` all-reduces of the n_txps count vector
 * back to back on the store's stream, between HIP events; *out_avg_us = microseconds per all-reduce
 * (the exchange by itself: peer to peer = publish + reduce kernels, RCCL = ncclAllReduce). */
int oem_time_allreduce(oem_store *store, uint32_t n_calls, float *out_avg_us);

/* Device time of the batched EM loops of this thread's LAST oem_em_run_cells call: milliseconds between
 * HIP events recorded on the group's stream right before the first and right after the last pass of
 * every batched group (upload, layout build and read-back excluded) -- groups that ran side by side on the
 * device (two workers) count the time they shared once: the length of the union of the groups' loops -- and
 * the batched passes launched, summed over the groups.
 * Together with the per-cell n_passes of `infos` this gives bench.py the roofline of the per-cell leg:
 * bytes = sum over cells of n_passes * (nnz_c * 8 + (R_c + 1) * 4 + 2 * T * 8).  Zero when every group
 * took the cell-by-cell fallback. */
int oem_cells_last_timing(float *out_loop_ms, uint64_t *out_batched_passes);

#ifdef __cplusplus
}
#endif
#endif /* OARFISH_EM_H */
