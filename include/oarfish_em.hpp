// oarfish_em.hpp -- C++17 host-side mirror of the reference's EM interface over the C ABI.
//
// The reference is compiled code (Rust); no Rust toolchain exists in this image, so the host
// side above include/oarfish_em.h is mirrored here in C++ with the reference's own names and
// argument meaning (COMBINE-lab/oarfish v0.10.3):
//
//   oarfish::AlnInfo                 src/util/oarfish_types.rs:330-337
//   oarfish::AlignmentFilters        src/util/oarfish_types.rs:763-806 (only model_coverage, :792)
//   oarfish::TranscriptInfo          src/util/oarfish_types.rs:431-437 (len / lenf)
//   oarfish::InMemoryAlignmentStore  src/util/oarfish_types.rs:548-558, add_filtered_group :718-738,
//                                    len :562-564, total_len / num_aligned_reads :741-748
//   oarfish::EMInfo                  src/util/oarfish_types.rs:408-428
//   oarfish::em::em / em_par / bootstrap   src/em.rs:262 / :320 / :292
//
// Error behaviour: the reference's EM is infallible (it aborts on a panic, Cargo.toml:118); here a
// failed call throws oarfish::OemError carrying the oem_status and message.  Header-only; link
// against liboarfish_em.so.
#pragma once

#include <cstdint>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "oarfish_em.h"

namespace oarfish {

struct OemError : std::runtime_error {
    int code;
    OemError(int c, const std::string &what) : std::runtime_error(what), code(c) {}
};

inline void check(int rc, const char *where)
{
    if (rc != OEM_OK) throw OemError(rc, std::string(where) + ": " + oem_last_error());
}

enum class Strand : uint8_t { Forward, Reverse, Unknown };

struct AlnInfo { // oarfish_types.rs:330-337
    uint32_t ref_id = 0;
    uint32_t start = 0;
    uint32_t end = 0;
    double prob = 0.0; // always 0.0 in the reference and never read (oarfish_types.rs:352)
    Strand strand = Strand::Forward;
    uint32_t alignment_span() const { return end - start; } // :341-343
};

struct AlignmentFilters {
    bool model_coverage = false; // oarfish_types.rs:792; selects the cov_prob column (em.rs:108)
};

struct TranscriptInfo { // oarfish_types.rs:431-437; the EM reads lenf only under --use-kde
    size_t len = 1;
    double total_weight = 0.0;
    double lenf = 1.0;
};

namespace detail {
struct StoreDeleter {
    void operator()(oem_store *s) const { oem_store_destroy(s); }
};
} // namespace detail

class InMemoryAlignmentStore { // oarfish_types.rs:548-558
public:
    AlignmentFilters filter_opts;
    std::vector<AlnInfo> alignments;
    std::vector<float> as_probabilities;
    std::vector<double> coverage_probabilities;

    explicit InMemoryAlignmentStore(AlignmentFilters fo = {}) : filter_opts(fo), boundaries_{0} {} // :637-649

    // :718-738 (the coverage intervals it also updates belong to the coverage model, out of scope)
    bool add_filtered_group(const std::vector<AlnInfo> &alns, const std::vector<float> &as_probs)
    {
        if (alns.empty()) return false;
        if (alns.size() != as_probs.size()) throw std::invalid_argument("add_filtered_group: sizes differ");
        alignments.insert(alignments.end(), alns.begin(), alns.end());
        as_probabilities.insert(as_probabilities.end(), as_probs.begin(), as_probs.end());
        coverage_probabilities.resize(alignments.size(), 0.0);
        boundaries_.push_back(alignments.size());
        device_.reset();
        return true;
    }
    size_t len() const { return boundaries_.size() - 1; }          // :562-564
    size_t num_aligned_reads() const { return len(); }             // :746-748
    size_t total_len() const { return alignments.size(); }         // :741-743
    // iter(): read i as (begin, end) into the three columns (:651-656)
    std::pair<size_t, size_t> read(size_t i) const { return {boundaries_[i], boundaries_[i + 1]}; }

    // The matrix resident in HBM (uploaded once, kept across em / bootstrap calls like the store
    // stays in RAM across bulk.rs:131-194).
    oem_store *device_store(size_t n_txps, int device = 0) const
    {
        if (!device_ || dev_txps_ != n_txps || dev_id_ != device) {
            std::vector<uint64_t> row_ptr(boundaries_.begin(), boundaries_.end());
            std::vector<uint32_t> tid(alignments.size());
            for (size_t j = 0; j < alignments.size(); ++j) tid[j] = alignments[j].ref_id;
            oem_store *h = nullptr;
            check(oem_store_create(row_ptr.data(), tid.data(), as_probabilities.data(),
                                   filter_opts.model_coverage ? coverage_probabilities.data() : nullptr, // em.rs:108
                                   len(), alignments.size(), (uint32_t)n_txps, device, nullptr, &h),
                  "oem_store_create");
            device_.reset(h);
            dev_txps_ = n_txps;
            dev_id_ = device;
        }
        return device_.get();
    }

private:
    std::vector<size_t> boundaries_; // private in the reference too (:555)
    mutable std::unique_ptr<oem_store, detail::StoreDeleter> device_;
    mutable size_t dev_txps_ = 0;
    mutable int dev_id_ = 0;
};

struct EMInfo { // oarfish_types.rs:408-428
    const InMemoryAlignmentStore *eq_map = nullptr;
    const std::vector<TranscriptInfo> *txp_info = nullptr;
    uint32_t max_iter = 1000;           // prog_opts.rs:532
    double convergence_thresh = 1e-3;   // prog_opts.rs:536
    std::optional<std::vector<double>> init_abundances;
    bool kde_model = false;             // hidden --use-kde: not supported (un-pinned kders crate)
    int device = 0;
};

// OEM_OPT_RUN_HISTORY: the store records the rel_diff of each loop pass of its next em / em_par / bootstrap calls, the
// first min(capacity, max_iter) passes of each run; 0 switches it off (the default).
inline void set_run_history(oem_store *store, uint32_t capacity)
{
    check(oem_store_set_option(store, OEM_OPT_RUN_HISTORY, capacity), "oem_store_set_option");
}

// The recorded rel_diff of run `run` of the last call on the store (0 after em / em_par, the replicate after
// bootstrap): entry N - 1 is the R of the reference's log line `iteration N; rel diff R` (em.rs:219-233, :405-419).
// *run_len (optional) receives the run's loop passes, which may exceed the entries stored.
inline std::vector<double> run_history(const oem_store *store, uint32_t run = 0, uint32_t *run_len = nullptr)
{
    uint32_t n = 0;
    uint64_t stored = 0;
    check(oem_run_history(store, run, nullptr, 0, &n), "oem_run_history");
    check(oem_store_info(store, OEM_INFO_RUN_HISTORY_STORED, &stored), "oem_store_info");
    std::vector<double> h(n < stored ? n : (size_t)stored);
    check(oem_run_history(store, run, h.data(), (uint32_t)h.size(), nullptr), "oem_run_history");
    if (run_len) *run_len = n;
    return h;
}

// write_function.rs:283-332: the body lines of the `.prob` file for every read of the store, formatted on the device
// (oem_assignment_text).  `names` holds one name per read (empty: every name is empty); *line_off / *kept (optional)
// receive the n_reads + 1 byte offsets of the lines and each line's k.
inline std::string assignment_text(oem_store *store, const std::vector<double> &counts, double display_thresh,
                                   const std::vector<std::string> &names = {}, std::vector<uint64_t> *line_off = nullptr,
                                   std::vector<uint32_t> *kept = nullptr)
{
    std::string blob;
    std::vector<uint64_t> off;
    if (!names.empty()) {
        off.reserve(names.size() + 1);
        off.push_back(0);
        for (const std::string &n : names) {
            blob += n;
            off.push_back(blob.size());
        }
    }
    oem_text_result *r = nullptr;
    check(oem_assignment_text(store, counts.data(), display_thresh,
                              names.empty() ? nullptr : reinterpret_cast<const uint8_t *>(blob.data()),
                              names.empty() ? nullptr : off.data(), &r),
          "oem_assignment_text");
    std::unique_ptr<oem_text_result, void (*)(oem_text_result *)> guard(r, oem_text_result_destroy);
    uint64_t n_bytes = 0, n_lines = 0;
    check(oem_text_result_dims(r, &n_bytes, &n_lines, nullptr), "oem_text_result_dims");
    std::string text(n_bytes, '\0');
    if (line_off) line_off->resize(n_lines + 1);
    if (kept) kept->resize(n_lines);
    check(oem_text_result_copy(r, reinterpret_cast<uint8_t *>(&text[0]), line_off ? line_off->data() : nullptr,
                               kept ? kept->data() : nullptr),
          "oem_text_result_copy");
    return text;
}

namespace em {

namespace detail {
inline std::vector<double> run(const EMInfo &emi, uint32_t gate, oem_run_info *info)
{
    if (emi.kde_model) throw std::invalid_argument("kde_model is not supported");
    const size_t T = emi.txp_info->size();
    oem_store *s = emi.eq_map->device_store(T, emi.device);
    std::vector<double> out(T, 0.0);
    check(oem_em_run(s, emi.init_abundances ? emi.init_abundances->data() : nullptr, emi.max_iter,
                     emi.convergence_thresh, gate, out.data(), info),
          "oem_em_run");
    return out;
}
} // namespace detail

// em.rs:262-271: `_nthreads` is ignored there too
inline std::vector<double> em(const EMInfo &em_info, size_t /*nthreads*/, oem_run_info *info = nullptr)
{
    return detail::run(em_info, 50, info); // gate niter > 50 (em.rs:212)
}

// em.rs:320-447
inline std::vector<double> em_par(const EMInfo &em_info, size_t /*nthreads*/, oem_run_info *info = nullptr)
{
    return detail::run(em_info, 1, info); // gate niter > 1 (em.rs:399)
}

// em.rs:292-314; `seed` keys the device RNG (the reference seeds from the OS, em.rs:274),
// `row_weights` (num_boot x n_reads multiplicities) injects the resamples.
inline std::vector<std::vector<double>> bootstrap(const EMInfo &em_info, uint32_t num_boot, size_t /*nthreads*/,
                                                  uint64_t seed = 0, const uint32_t *row_weights = nullptr)
{
    if (em_info.kde_model) throw std::invalid_argument("kde_model is not supported");
    const size_t T = em_info.txp_info->size();
    oem_store *s = em_info.eq_map->device_store(T, em_info.device);
    std::vector<double> flat((size_t)num_boot * T, 0.0);
    check(oem_bootstrap(s, num_boot, seed, row_weights,
                        em_info.init_abundances ? em_info.init_abundances->data() : nullptr, em_info.max_iter,
                        em_info.convergence_thresh, flat.data(), nullptr),
          "oem_bootstrap");
    std::vector<std::vector<double>> out(num_boot);
    for (uint32_t b = 0; b < num_boot; ++b) out[b].assign(flat.begin() + (size_t)b * T, flat.begin() + (size_t)(b + 1) * T);
    return out;
}

} // namespace em
} // namespace oarfish
