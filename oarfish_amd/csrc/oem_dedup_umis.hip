// oem_dedup_umis.hip -- UMI deduplication on the device: oem_dedup_umis, and the stages the one call
// oem_em_run_cells_records_umis_sparse (oem_cells_records.hip) runs between a group's name collation and its record gather.
//
// The rule is oem_collate.h's ("UMI deduplication"); nothing of it is in the reference, whose documentation wants the
// input deduplicated already (docs/index.md:308-312).  The whole input's UMIs are resident, in input order, validated
// behind their upload chunks (umis_upload: a 0 byte is an error, an empty UMI is legal).  Then, per batch of cells whose
// order, group_off and cell_group_off are on the device (dedup_mark):
//   heads      k_umi_heads: a group's head input index (through order_bc where the order still holds positions of the
//              barcode collation) and whether the group takes part -- it has a record, its head's UMI is not empty, its
//              head is not unmapped
//   scan       the exclusive scan of "takes part" numbers the participants; sampled at the cells' first groups it is the
//              participants' cell offsets (k_umi_sample), the only thing of this stage the host reads
//   gather     k_umi_part closes ranks (the participants' heads and groups), gather_name_offsets / gather_names put
//              their UMIs into one dense padded blob
//   collate    collate_resident in its device form over that blob: the cells are the cells, there are no secondary
//              flags, so the start order is the participants' own and every sort is stable -- its runs are the classes,
//              and a run's first element is its smallest group, the survivor
//   mark       k_umi_mark: every element of a run but the first is a duplicate of the first
//   counts     the exclusive scan of "is no duplicate" is the groups' new numbers; k_umi_cell_dups samples it per cell
// and, where the caller goes on with the collation (dedup_compact): one more scan, of the duplicates' record counts, and
// k_umi_compact writes order', group_off', cell_group_off' and the cells' first positions.  A batch without a
// participant, or without a duplicate, leaves after the first scan or after the mark with nothing moved.
//
// All kernels are wave64, one lane per element, plain loads and vector stores; the only atomics are the two atomicMin of
// the argument checks.  Everything runs on the null stream (collate_resident on its own) and leaves the device idle.
#include <hipcub/hipcub.hpp>

#include "oem_collate_device.h"
#include "oem_filter_device.h"

namespace oem {

namespace {

constexpr int kUT = 256;

__device__ __forceinline__ uint64_t tid64() { return (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; }
inline dim3 grid_for(uint64_t n) { return dim3((unsigned)std::max<uint64_t>((n + kUT - 1) / kUT, 1)); }

// the last r < n with off[r] <= p (off[0] <= p): the run of a position, the group of a position
__device__ __forceinline__ uint64_t last_at_or_before(const uint64_t *__restrict__ off, uint64_t n, uint64_t p)
{
    uint64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// oem_dedup_umis: the smallest position of the call whose order entry is not below n_records -> *bad
__global__ __launch_bounds__(kUT) void k_umi_check_order(uint64_t m, const uint32_t *__restrict__ order, uint64_t n_records, uint64_t pos_base,
                                                          unsigned long long *__restrict__ bad)
{
    const uint64_t k = tid64();
    if (k < m && order[k] >= n_records) atomicMin(bad, (unsigned long long)(pos_base + k));
}

// group g < ng: head[g], part[g] (1 when the group takes part; part[ng] = 0, for the scan), keep[g] = 1 (keep[ng] = 0),
// dup[g] = 0, survivor[g] = survivor_base + g
__global__ __launch_bounds__(kUT) void k_umi_heads(uint64_t ng, const uint32_t *__restrict__ order, const uint32_t *__restrict__ order_bc,
                                                    const uint64_t *__restrict__ group_off, const uint64_t *__restrict__ umi_off,
                                                    const uint32_t *__restrict__ flags, uint64_t flags_stride, uint64_t survivor_base,
                                                    uint32_t *__restrict__ head, uint64_t *__restrict__ part, uint64_t *__restrict__ keep,
                                                    uint32_t *__restrict__ dup, uint64_t *__restrict__ survivor)
{
    const uint64_t g = tid64();
    if (g > ng) return;
    if (g == ng) {
        part[g] = 0;
        keep[g] = 0;
        return;
    }
    const uint64_t p0 = group_off[g], p1 = group_off[g + 1];
    uint32_t h = 0;
    bool take = false;
    if (p1 > p0) {
        h = order[p0];
        if (order_bc) h = order_bc[h];
        take = umi_off[(uint64_t)h + 1] > umi_off[h] && !(flags && (flags[(uint64_t)h * flags_stride] & kRecUnmapped));
    }
    head[g] = h;
    part[g] = take ? 1ull : 0ull;
    keep[g] = 1ull;
    dup[g] = 0u;
    survivor[g] = survivor_base + g;
}

// pidx: the exclusive scan of part.  The participants close ranks: their heads and their groups.
__global__ __launch_bounds__(kUT) void k_umi_part(uint64_t ng, const uint64_t *__restrict__ part, const uint64_t *__restrict__ pidx,
                                                   const uint32_t *__restrict__ head, uint32_t *__restrict__ phead, uint32_t *__restrict__ pgroup)
{
    const uint64_t g = tid64();
    if (g >= ng || !part[g]) return;
    phead[pidx[g]] = head[g];
    pgroup[pidx[g]] = (uint32_t)g;
}

// dst[c] = scan[cell_group_off[c]] for the nc + 1 cell boundaries
__global__ __launch_bounds__(kUT) void k_umi_sample(uint64_t n, const uint64_t *__restrict__ cell_group_off, const uint64_t *__restrict__ scan,
                                                     uint64_t *__restrict__ dst)
{
    const uint64_t c = tid64();
    if (c < n) dst[c] = scan[cell_group_off[c]];
}

// uorder: the participants in (cell, UMI bytes, participant) order; run_off (n_runs + 1): where a class starts.  Every
// element of a run but its first is a duplicate of the first.
__global__ __launch_bounds__(kUT) void k_umi_mark(uint64_t n_part, const uint32_t *__restrict__ uorder, const uint64_t *__restrict__ run_off,
                                                   uint64_t n_runs, const uint32_t *__restrict__ pgroup, uint64_t survivor_base,
                                                   uint32_t *__restrict__ dup, uint64_t *__restrict__ keep, uint64_t *__restrict__ survivor)
{
    const uint64_t p = tid64();
    if (p >= n_part) return;
    const uint64_t first = run_off[last_at_or_before(run_off, n_runs, p)];
    if (first == p) return;
    const uint32_t g = pgroup[uorder[p]];
    dup[g] = 1u;
    keep[g] = 0ull;
    survivor[g] = survivor_base + pgroup[uorder[first]];
}

// gscan: the exclusive scan of keep.  cell_dups[c] = the groups of cell c that are not kept.
__global__ __launch_bounds__(kUT) void k_umi_cell_dups(uint64_t nc, const uint64_t *__restrict__ cell_group_off, const uint64_t *__restrict__ gscan,
                                                        uint64_t *__restrict__ cell_dups)
{
    const uint64_t c = tid64();
    if (c >= nc) return;
    const uint64_t g0 = cell_group_off[c], g1 = cell_group_off[c + 1];
    cell_dups[c] = (g1 - g0) - (gscan[g1] - gscan[g0]);
}

// rlen[g] = the records of group g if it is a duplicate, else 0; rlen[ng] = 0
__global__ __launch_bounds__(kUT) void k_umi_removed(uint64_t ng, const uint32_t *__restrict__ dup, const uint64_t *__restrict__ group_off,
                                                      uint64_t *__restrict__ rlen)
{
    const uint64_t g = tid64();
    if (g > ng) return;
    rlen[g] = g < ng && dup[g] ? group_off[g + 1] - group_off[g] : 0ull;
}

// gscan: the kept groups' new numbers; rscan: the exclusive scan of rlen, the positions removed before a group.  One
// lane per position, per group boundary and per cell boundary, whichever the index still covers.
__global__ __launch_bounds__(kUT) void k_umi_compact(uint64_t m, uint64_t ng, uint64_t nc, const uint32_t *__restrict__ order,
                                                      const uint64_t *__restrict__ group_off, const uint64_t *__restrict__ cell_group_off,
                                                      const uint32_t *__restrict__ dup, const uint64_t *__restrict__ gscan,
                                                      const uint64_t *__restrict__ rscan, uint32_t *__restrict__ order_out,
                                                      uint64_t *__restrict__ group_off_out, uint64_t *__restrict__ cell_group_off_out,
                                                      uint64_t *__restrict__ cell_pos_out)
{
    const uint64_t k = tid64();
    if (k < m) {
        const uint64_t g = last_at_or_before(group_off, ng, k);
        if (!dup[g]) order_out[k - rscan[g]] = order[k];
    }
    if (k < ng && !dup[k]) group_off_out[gscan[k]] = group_off[k] - rscan[k];
    if (k == ng) group_off_out[gscan[ng]] = m - rscan[ng];
    if (k <= nc) {
        const uint64_t g = cell_group_off[k];
        cell_group_off_out[k] = gscan[g];
        cell_pos_out[k] = group_off[g] - rscan[g];
    }
}

// out = the exclusive scan of in, n items, on the null stream; tmp only grows
struct ScanTmp {
    void *p = nullptr;
    size_t cap = 0;
    ~ScanTmp() { (void)hipFree(p); }
};
int exclusive_sum(ScanTmp &t, const uint64_t *in, uint64_t *out, uint64_t n)
{
    size_t tb = 0;
    OEM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, (int)n, nullptr));
    if (tb > t.cap || !t.p) {
        OEM_HIP(hipStreamSynchronize(nullptr));
        (void)hipFree(t.p);
        t.p = nullptr;
        t.cap = 0;
        OEM_HIP(hipMalloc(&t.p, tb ? tb : 1));
        t.cap = tb ? tb : 1;
    }
    tb = t.cap;
    OEM_HIP(hipcub::DeviceScan::ExclusiveSum(t.p, tb, in, out, (int)n, nullptr));
    return OEM_OK;
}

} // namespace

int umis_upload(const char *who, const uint8_t *umis, const uint64_t *umi_off, uint64_t n, DevBuf<uint8_t> *d_umis, DevBuf<uint64_t> *d_umi_off)
{
    const uint64_t n_bytes = umi_off[n], chunk_bytes = collate_chunk_bytes();
    DevBuf<unsigned long long> d_bad;
    OEM_TRY(dev_alloc(&d_umis->p, n_bytes + 16, nullptr));
    OEM_TRY(dev_alloc(&d_umi_off->p, n + 1, nullptr));
    OEM_TRY(dev_alloc(&d_bad.p, 2, nullptr));
    const unsigned long long bad0[2] = {kNoRecord, kNoRecord};
    OEM_HIP(hipMemcpy(d_bad.p, bad0, sizeof bad0, hipMemcpyHostToDevice));
    OEM_HIP(hipMemcpy(d_umi_off->p, umi_off, sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice));
    OEM_HIP(hipMemset(d_umis->p + n_bytes, 0, 16));
    if (!n_bytes) return OEM_OK;
    std::vector<uint64_t> byte_cut{0}, rec_cut{0};
    for (uint64_t r = 0; r < n;) { // cut wherever a record ends; the records behind the last byte go with the last chunk
        uint64_t r1 = (uint64_t)(std::upper_bound(umi_off + r + 1, umi_off + n + 1, umi_off[r] + chunk_bytes) - umi_off) - 1;
        r1 = std::max(r1, r + 1);
        byte_cut.push_back(umi_off[r1]);
        rec_cut.push_back(r1);
        r = r1;
    }
    // the validate kernel of the names: its empty-name word (d_bad[1]) is not read here, an empty UMI being legal
    OEM_TRY(filter_upload_measure<uint8_t>(umis, d_umis->p, byte_cut.data(), byte_cut.size() - 1, 1, nullptr,
                                           [&](hipStream_t lane, uint64_t g0, uint64_t) {
                                               launch_collate_validate(lane, d_umis->p, byte_cut[g0], byte_cut[g0 + 1], d_umi_off->p,
                                                                       rec_cut[g0], rec_cut[g0 + 1], d_bad.p);
                                           }));
    unsigned long long bad[2];
    OEM_HIP(hipMemcpy(bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost));
    if (bad[0] != kNoRecord) return fail(OEM_ERR_ARG, "%s: the UMI of record %llu contains a 0 byte", who, bad[0]);
    return OEM_OK;
}

int umis_gather_survivors(const uint8_t *d_umis, const uint64_t *d_umi_off, const uint32_t *d_order, uint64_t m, DevBuf<uint8_t> *d_dense,
                          DevBuf<uint64_t> *d_dense_off, uint64_t *dense_bytes, uint64_t *bad_record)
{
    *bad_record = kNoRecord;
    DevBuf<unsigned long long> d_bad;
    OEM_TRY(dev_alloc(&d_bad.p, 2, nullptr));
    const unsigned long long bad0[2] = {kNoRecord, kNoRecord};
    OEM_HIP(hipMemcpy(d_bad.p, bad0, sizeof bad0, hipMemcpyHostToDevice));
    OEM_TRY(dev_alloc(&d_dense_off->p, m + 1, nullptr));
    OEM_TRY(gather_name_offsets(d_order, m, d_umi_off, d_dense_off->p));
    OEM_HIP(hipMemcpy(dense_bytes, d_dense_off->p + m, sizeof *dense_bytes, hipMemcpyDeviceToHost));
    OEM_TRY(dev_alloc(&d_dense->p, *dense_bytes + 16, nullptr));
    OEM_TRY(gather_names(d_order, m, d_umis, d_umi_off, d_dense_off->p, 0, *dense_bytes, d_dense->p, nullptr, nullptr, true));
    if (!*dense_bytes) return OEM_OK;
    // (the validate kernel of the names: its empty-name word is not read, an empty UMI being legal)
    launch_collate_validate(nullptr, d_dense->p, 0, *dense_bytes, d_dense_off->p, 0, m, d_bad.p);
    OEM_HIP(hipGetLastError());
    unsigned long long bad[2];
    OEM_HIP(hipMemcpy(bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost));
    if (bad[0] != kNoRecord) {
        uint32_t record = 0;
        OEM_HIP(hipMemcpy(&record, d_order + bad[0], sizeof record, hipMemcpyDeviceToHost));
        *bad_record = record;
    }
    return OEM_OK;
}

int dedup_mark(const UmiInput &in, const uint32_t *d_order, const uint32_t *d_order_bc, const uint64_t *d_group_off, uint64_t ng,
               const uint64_t *d_cell_group_off, uint32_t nc, uint64_t survivor_base, UmiMarks *out, uint64_t *cell_dups)
{
    std::fill(cell_dups, cell_dups + nc, 0ull);
    out->n_part = out->n_classes = out->n_dups = 0;
    if (!ng) return OEM_OK;
    ScanTmp tmp;
    DevBuf<uint32_t> d_head, d_phead, d_pgroup;
    DevBuf<uint64_t> d_part, d_pidx, d_pcell, d_poff, d_cell_dups;
    DevBuf<uint8_t> d_blob;
    OEM_TRY(dev_alloc(&out->dup.p, ng, nullptr));
    OEM_TRY(dev_alloc(&out->survivor.p, ng, nullptr));
    OEM_TRY(dev_alloc(&out->keep.p, ng + 1, nullptr));
    OEM_TRY(dev_alloc(&d_head.p, ng, nullptr));
    OEM_TRY(dev_alloc(&d_part.p, ng + 1, nullptr));
    OEM_TRY(dev_alloc(&d_pidx.p, ng + 1, nullptr));
    OEM_TRY(dev_alloc(&d_pcell.p, (size_t)nc + 1, nullptr));
    hipLaunchKernelGGL(k_umi_heads, grid_for(ng + 1), dim3(kUT), 0, nullptr, ng, d_order, d_order_bc, d_group_off, in.d_umi_off, in.d_flags,
                       in.flags_stride, survivor_base, d_head.p, d_part.p, out->keep.p, out->dup.p, out->survivor.p);
    OEM_HIP(hipGetLastError());
    OEM_TRY(exclusive_sum(tmp, d_part.p, d_pidx.p, ng + 1));
    hipLaunchKernelGGL(k_umi_sample, grid_for((uint64_t)nc + 1), dim3(kUT), 0, nullptr, (uint64_t)nc + 1, d_cell_group_off,
                       (const uint64_t *)d_pidx.p, d_pcell.p);
    OEM_HIP(hipGetLastError());
    std::vector<uint64_t> pcell((size_t)nc + 1);
    OEM_HIP(hipMemcpy(pcell.data(), d_pcell.p, sizeof(uint64_t) * ((size_t)nc + 1), hipMemcpyDeviceToHost));
    const uint64_t n_part = pcell[nc];
    out->n_part = n_part;
    if (n_part < 2) return OEM_OK; // (no two participants: no class has a second member)

    // the participants' heads and groups, and their UMIs as one dense blob
    OEM_TRY(dev_alloc(&d_phead.p, n_part, nullptr));
    OEM_TRY(dev_alloc(&d_pgroup.p, n_part, nullptr));
    OEM_TRY(dev_alloc(&d_poff.p, n_part + 1, nullptr));
    hipLaunchKernelGGL(k_umi_part, grid_for(ng), dim3(kUT), 0, nullptr, ng, (const uint64_t *)d_part.p, (const uint64_t *)d_pidx.p,
                       (const uint32_t *)d_head.p, d_phead.p, d_pgroup.p);
    OEM_HIP(hipGetLastError());
    OEM_TRY(gather_name_offsets(d_phead.p, n_part, in.d_umi_off, d_poff.p));
    uint64_t nb = 0;
    OEM_HIP(hipMemcpy(&nb, d_poff.p + n_part, sizeof nb, hipMemcpyDeviceToHost));
    d_head.reset();
    d_part.reset();
    d_pidx.reset();
    OEM_TRY(dev_alloc(&d_blob.p, nb + 16, nullptr));
    OEM_TRY(gather_names(d_phead.p, n_part, in.d_umis, in.d_umi_off, d_poff.p, 0, nb, d_blob.p, nullptr, nullptr));
    d_phead.reset();

    // the classes: the runs of the name collation over the UMIs, the cells being the cells
    CollateInput cc;
    cc.who = in.who;
    cc.what = "UMI";
    cc.cell_rec_off = pcell.data();
    cc.mode = kCollateSort;
    cc.chunk_bytes = collate_chunk_bytes();
    cc.d_names = d_blob.p;
    cc.d_name_off = d_poff.p;
    cc.d_off_base = 0;
    cc.d_n_bytes = nb;
    CollateResident ucr;
    double info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    OEM_TRY(collate_resident(cc, 0, nc, 0, 0, 0, info, &ucr));
    d_blob.reset();
    d_poff.reset();
    out->n_classes = ucr.n_groups;
    out->n_dups = n_part - ucr.n_groups;
    if (!out->n_dups) return OEM_OK;

    hipLaunchKernelGGL(k_umi_mark, grid_for(n_part), dim3(kUT), 0, nullptr, n_part, (const uint32_t *)ucr.order.p,
                       (const uint64_t *)ucr.group_off.p, ucr.n_groups, (const uint32_t *)d_pgroup.p, survivor_base, out->dup.p, out->keep.p,
                       out->survivor.p);
    OEM_HIP(hipGetLastError());
    OEM_TRY(dev_alloc(&out->gscan.p, ng + 1, nullptr));
    OEM_TRY(dev_alloc(&d_cell_dups.p, nc, nullptr));
    OEM_TRY(exclusive_sum(tmp, out->keep.p, out->gscan.p, ng + 1));
    hipLaunchKernelGGL(k_umi_cell_dups, grid_for(nc), dim3(kUT), 0, nullptr, (uint64_t)nc, d_cell_group_off, (const uint64_t *)out->gscan.p,
                       d_cell_dups.p);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipMemcpy(cell_dups, d_cell_dups.p, sizeof(uint64_t) * nc, hipMemcpyDeviceToHost));
    return OEM_OK;
}

int dedup_compact(const UmiMarks &mk, uint64_t m, uint32_t nc, CollateResident *cr, uint64_t *n_positions, uint64_t *cell_pos_off)
{
    const uint64_t ng = cr->n_groups;
    ScanTmp tmp;
    DevBuf<uint64_t> d_rlen, d_rscan, d_goff, d_cgo, d_cpos;
    DevBuf<uint32_t> d_order;
    OEM_TRY(dev_alloc(&d_rlen.p, ng + 1, nullptr));
    OEM_TRY(dev_alloc(&d_rscan.p, ng + 1, nullptr));
    hipLaunchKernelGGL(k_umi_removed, grid_for(ng + 1), dim3(kUT), 0, nullptr, ng, (const uint32_t *)mk.dup.p, (const uint64_t *)cr->group_off.p,
                       d_rlen.p);
    OEM_HIP(hipGetLastError());
    OEM_TRY(exclusive_sum(tmp, d_rlen.p, d_rscan.p, ng + 1));
    uint64_t removed = 0;
    OEM_HIP(hipMemcpy(&removed, d_rscan.p + ng, sizeof removed, hipMemcpyDeviceToHost));
    d_rlen.reset();
    const uint64_t m_out = m - removed, ng_out = ng - mk.n_dups;
    OEM_TRY(dev_alloc(&d_order.p, m_out, nullptr));
    OEM_TRY(dev_alloc(&d_goff.p, ng_out + 1, nullptr));
    OEM_TRY(dev_alloc(&d_cgo.p, (size_t)nc + 1, nullptr));
    OEM_TRY(dev_alloc(&d_cpos.p, (size_t)nc + 1, nullptr));
    hipLaunchKernelGGL(k_umi_compact, grid_for(std::max<uint64_t>(m, std::max<uint64_t>(ng + 1, (uint64_t)nc + 1))), dim3(kUT), 0, nullptr, m, ng,
                       (uint64_t)nc, (const uint32_t *)cr->order.p, (const uint64_t *)cr->group_off.p, (const uint64_t *)cr->cell_group_off.p,
                       (const uint32_t *)mk.dup.p, (const uint64_t *)mk.gscan.p, (const uint64_t *)d_rscan.p, d_order.p, d_goff.p, d_cgo.p,
                       d_cpos.p);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipMemcpy(cell_pos_off, d_cpos.p, sizeof(uint64_t) * ((size_t)nc + 1), hipMemcpyDeviceToHost));
    std::swap(cr->order.p, d_order.p);
    std::swap(cr->group_off.p, d_goff.p);
    std::swap(cr->cell_group_off.p, d_cgo.p);
    cr->n_groups = ng_out;
    *n_positions = m_out;
    return OEM_OK;
}

} // namespace oem

using namespace oem;

extern "C" int oem_dedup_umis(const uint8_t *umis, const uint64_t *umi_off, const uint32_t *flags, uint64_t n_records, const uint32_t *order,
                              uint64_t n_positions, const uint64_t *group_off, uint64_t n_groups, const uint64_t *cell_group_off,
                              uint32_t n_cells, int device, uint8_t *out_dup, uint64_t *out_survivor, uint64_t *out_cell_dups)
{
    OEM_API_BEGIN
    const char *who = "oem_dedup_umis";
    if (!umi_off || !group_off || !cell_group_off || !out_dup || !out_survivor || !out_cell_dups)
        return fail(OEM_ERR_ARG, "%s: umi_off, group_off, cell_group_off or an output is NULL", who);
    if (n_records > 0xffffffffull) return fail(OEM_ERR_ARG, "%s: %llu records: more than 2^32 - 1", who, (unsigned long long)n_records);
    if (n_positions > 0xffffffffull) return fail(OEM_ERR_ARG, "%s: %llu positions: more than 2^32 - 1", who, (unsigned long long)n_positions);
    OEM_TRY(check_offsets(who, "umi_off", umi_off, n_records, "record"));
    if (umi_off[n_records] && !umis) return fail(OEM_ERR_ARG, "%s: umis is NULL and the UMIs are not all empty", who);
    if (n_positions && !order) return fail(OEM_ERR_ARG, "%s: order is NULL and n_positions is not 0", who);
    OEM_TRY(check_offsets(who, "group_off", group_off, n_groups, "group"));
    if (group_off[n_groups] != n_positions)
        return fail(OEM_ERR_ARG, "%s: group_off ends at %llu, not at n_positions = %llu", who, (unsigned long long)group_off[n_groups],
                    (unsigned long long)n_positions);
    OEM_TRY(check_offsets(who, "cell_group_off", cell_group_off, n_cells, "cell"));
    if (cell_group_off[n_cells] != n_groups)
        return fail(OEM_ERR_ARG, "%s: cell_group_off ends at %llu, not at n_groups = %llu", who, (unsigned long long)cell_group_off[n_cells],
                    (unsigned long long)n_groups);
    for (uint32_t c = 0; c < n_cells; ++c)
        if (group_off[cell_group_off[c + 1]] - group_off[cell_group_off[c]] > kCollateMaxBatch)
            return fail(OEM_ERR_ARG, "%s: cell %u has more than 2^31 - 2 records", who, c);
    for (uint32_t c = 0; c < n_cells; ++c)
        if (cell_group_off[c + 1] - cell_group_off[c] > kCollateMaxBatch)
            return fail(OEM_ERR_ARG, "%s: cell %u has more than 2^31 - 2 groups", who, c);
    OEM_TRY(ensure_device(device));

    for (uint64_t g = 0; g < n_groups; ++g) {
        out_dup[g] = 0;
        out_survivor[g] = g;
    }
    std::fill(out_cell_dups, out_cell_dups + n_cells, 0ull);
    if (!n_groups || !n_positions) return OEM_OK;

    // the UMIs and the flags, once and in input order; the order's entries are checked as it goes up
    DevBuf<uint8_t> d_umis;
    DevBuf<uint64_t> d_umi_off;
    DevBuf<uint32_t> d_flags, d_order;
    DevBuf<unsigned long long> d_bad;
    OEM_TRY(dev_alloc(&d_order.p, n_positions, nullptr));
    OEM_TRY(dev_alloc(&d_bad.p, 1, nullptr));
    const unsigned long long none = kNoRecord;
    OEM_HIP(hipMemcpy(d_bad.p, &none, sizeof none, hipMemcpyHostToDevice));
    OEM_HIP(hipMemcpy(d_order.p, order, sizeof(uint32_t) * n_positions, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_umi_check_order, grid_for(n_positions), dim3(kUT), 0, nullptr, n_positions, (const uint32_t *)d_order.p, n_records,
                       (uint64_t)0, d_bad.p);
    OEM_HIP(hipGetLastError());
    unsigned long long bad = kNoRecord;
    OEM_HIP(hipMemcpy(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost));
    if (bad != kNoRecord)
        return fail(OEM_ERR_ARG, "%s: order[%llu] = %u is not below n_records = %llu", who, bad, order[bad], (unsigned long long)n_records);
    OEM_TRY(umis_upload(who, umis, umi_off, n_records, &d_umis, &d_umi_off));
    if (!umi_off[n_records]) return OEM_OK; // every UMI is empty: no group takes part
    if (flags) {
        OEM_TRY(dev_alloc(&d_flags.p, n_records, nullptr));
        OEM_HIP(hipMemcpy(d_flags.p, flags, sizeof(uint32_t) * n_records, hipMemcpyHostToDevice));
    }
    UmiInput in;
    in.who = who;
    in.d_umis = d_umis.p;
    in.d_umi_off = d_umi_off.p;
    in.d_flags = d_flags.p;
    in.flags_stride = 1;

    // batches of whole cells, as oem_collate_names cuts them: the offsets go up rebased to the batch
    const uint64_t batch_records = collate_batch_records();
    std::vector<uint64_t> goff, cgo;
    std::vector<uint32_t> dup;
    for (uint32_t c0 = 0; c0 < n_cells;) {
        uint32_t c1 = c0 + 1;
        while (c1 < n_cells && group_off[cell_group_off[c1 + 1]] - group_off[cell_group_off[c0]] <= batch_records &&
               cell_group_off[c1 + 1] - cell_group_off[c0] <= kCollateMaxBatch) // (groups without records count for the scans)
            ++c1;
        const uint64_t g0 = cell_group_off[c0], ng = cell_group_off[c1] - g0, p0 = group_off[g0];
        if (ng) {
            goff.resize(ng + 1);
            cgo.resize((size_t)(c1 - c0) + 1);
            for (uint64_t g = 0; g <= ng; ++g) goff[g] = group_off[g0 + g] - p0;
            for (uint32_t c = c0; c <= c1; ++c) cgo[c - c0] = cell_group_off[c] - g0;
            DevBuf<uint64_t> d_goff, d_cgo;
            OEM_TRY(dev_alloc(&d_goff.p, ng + 1, nullptr));
            OEM_TRY(dev_alloc(&d_cgo.p, cgo.size(), nullptr));
            OEM_HIP(hipMemcpy(d_goff.p, goff.data(), sizeof(uint64_t) * (ng + 1), hipMemcpyHostToDevice));
            OEM_HIP(hipMemcpy(d_cgo.p, cgo.data(), sizeof(uint64_t) * cgo.size(), hipMemcpyHostToDevice));
            UmiMarks mk;
            OEM_TRY(dedup_mark(in, d_order.p + p0, nullptr, d_goff.p, ng, d_cgo.p, c1 - c0, g0, &mk, out_cell_dups + c0));
            if (mk.n_dups) {
                dup.resize(ng);
                OEM_HIP(hipMemcpy(dup.data(), mk.dup.p, sizeof(uint32_t) * ng, hipMemcpyDeviceToHost));
                for (uint64_t g = 0; g < ng; ++g) out_dup[g0 + g] = dup[g] ? 1 : 0;
                OEM_HIP(hipMemcpy(out_survivor + g0, mk.survivor.p, sizeof(uint64_t) * ng, hipMemcpyDeviceToHost));
            }
        }
        c0 = c1;
    }
    return OEM_OK;
    OEM_API_END("oem_dedup_umis")
}
