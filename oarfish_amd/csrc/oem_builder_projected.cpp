// oem_builder_projected.cpp -- the host caller of oem_filter_projected.h: genome-mode reads into the store builder.
//
// Reference: InMemoryAlignmentStore::add_projected_group (src/util/oarfish_types.rs:695-715) runs
// AlignmentFilters::filter_projected (:1179-1297) and add_filtered_group (:718-738).  The per-read rule lives in
// oem_filter_projected.h, shared with the kernels of oem_filter_projected_device.hip; this file appends what it keeps to
// the same arrays oem_builder.cpp's add_group fills, one read (oem_builder_add_projected_group) or a batch
// (oem_builder_add_projected_groups) per call.  as_prob = expf(f) with libm's expf, which is what Rust's f32::exp is.
#include <cmath>
#include <vector>

#include "oem_driver.h"
#include "oem_filter_projected.h"

using namespace oem;

// One read: the discard table is touched only once no argument error is left (`first`: the index of the group's first
// record in the caller's array, ~0 for the single-group call).
static int add_one_projected_group(oem_builder *b, const oem_proj_record *ag, uint32_t n, uint64_t read_len,
                                   const oem_proj_opts &P, uint32_t *out_kept, const char *who, uint64_t first)
{
    if (out_kept) *out_kept = 0;
    const uint32_t T = (uint32_t)b->txp_len.size();
    FilterCounts c;
    const ProjGroup g = proj_group_measure(b->f, ag, n, read_len, b->txp_len.data(), T, c);
    if (g.flags & kFilterFlagBadRef) {
        const uint32_t ref = ag[g.bad_record].ref_id;
        const char *what = ref >= T ? "is not below n_txps" : "names a transcript of length 0";
        if (first == ~0ull) return fail(OEM_ERR_ARG, "%s: ref_id %u %s", who, ref, what);
        return fail(OEM_ERR_ARG, "%s: record %llu: ref_id %u %s", who, (unsigned long long)(first + g.bad_record), ref, what);
    }
    add_counts(b->dt, c);
    if (g.verdict != kProjValid || g.n_kept == 0) return OEM_OK;
    proj_group_emit(b->f, P, ag, n, b->txp_len.data(), T, g.best_sim, g.best_score,
                    [&](uint32_t, uint32_t, const oem_proj_record &x, uint32_t start, uint32_t end, float f) {
                        b->as_prob.push_back(expf(f));                                     // f.exp() (:1282)
                        b->tid.push_back(x.ref_id);                                        // AlnInfo (:1283-1293)
                        b->start.push_back(start);
                        b->end.push_back(end);
                        b->strand.push_back((x.flags & OEM_REC_REVERSE) ? 1 : 0);
                    });
    b->row_ptr.push_back(b->tid.size());                                                   // add_filtered_group (:724-735)
    if (out_kept) *out_kept = g.n_kept;
    return OEM_OK;
}

namespace oem {

int check_projected_batch(const char *who, const oem_proj_record *records, const uint64_t *group_off,
                          const uint64_t *read_len, uint64_t n_groups, const oem_proj_opts *popts)
{
    if (!popts) return fail(OEM_ERR_ARG, "%s: popts is NULL", who);
    if (!proj_source_ok(popts->prob_source))
        return fail(OEM_ERR_ARG, "%s: prob_source %d (0 similarity, 1 score or 2 combined)", who, popts->prob_source);
    OEM_TRY(check_group_off(who, records, group_off, n_groups));
    if (n_groups && !read_len) return fail(OEM_ERR_ARG, "%s: read_len is NULL", who);
    return OEM_OK;
}

int add_projected_groups_host(oem_builder *b, const oem_proj_record *records, const uint64_t *group_off,
                              const uint64_t *read_len, uint64_t n_groups, const oem_proj_opts &popts, uint32_t *out_kept,
                              const char *who)
{
    const BuilderMark mark = builder_mark(b);
    int rc = OEM_OK;
    try {
        for (uint64_t g = 0; g < n_groups && rc == OEM_OK; ++g)
            rc = add_one_projected_group(b, records + group_off[g], (uint32_t)(group_off[g + 1] - group_off[g]), read_len[g],
                                         popts, out_kept ? out_kept + g : nullptr, who, group_off[g]);
    } catch (...) {
        builder_rollback(b, mark);
        throw;
    }
    if (rc != OEM_OK) builder_rollback(b, mark);
    return rc;
}

} // namespace oem

extern "C" int oem_builder_add_projected_group(oem_builder *b, const oem_proj_record *ag, uint32_t n, uint64_t read_len,
                                               const oem_proj_opts *popts, uint32_t *out_kept)
{
    OEM_API_BEGIN
    const char *who = "oem_builder_add_projected_group";
    if (!b || (n && !ag)) return fail(OEM_ERR_ARG, "%s: NULL argument", who);
    if (!popts) return fail(OEM_ERR_ARG, "%s: popts is NULL", who);
    if (!proj_source_ok(popts->prob_source))
        return fail(OEM_ERR_ARG, "%s: prob_source %d (0 similarity, 1 score or 2 combined)", who, popts->prob_source);
    const BuilderMark mark = builder_mark(b);
    try {
        const int rc = add_one_projected_group(b, ag, n, read_len, *popts, out_kept, who, ~0ull);
        if (rc != OEM_OK) builder_rollback(b, mark);
        return rc;
    } catch (...) {
        builder_rollback(b, mark);
        throw;
    }
    OEM_API_END("oem_builder_add_projected_group")
}

extern "C" int oem_builder_add_projected_groups(oem_builder *b, const oem_proj_record *records, const uint64_t *group_off,
                                                const uint64_t *read_len, uint64_t n_groups, const oem_proj_opts *popts,
                                                uint32_t *out_kept)
{
    OEM_API_BEGIN
    const char *who = "oem_builder_add_projected_groups";
    if (!b) return fail(OEM_ERR_ARG, "%s: builder is NULL", who);
    OEM_TRY(check_projected_batch(who, records, group_off, read_len, n_groups, popts));
    return add_projected_groups_host(b, records, group_off, read_len, n_groups, *popts, out_kept, who);
    OEM_API_END("oem_builder_add_projected_groups")
}
