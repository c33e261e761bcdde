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
// Under a UMI rule (gene_of, correct; oem_dedup_umis_rule, oem_em_run_cells_records_umis_rule_sparse) the same stages run
// with
//   genes      k_umi_genes: gene(g) of every participant through its head's ref_id; the smallest head whose ref_id is not
//              below n_txps by atomicMin, as the order check reports
//   prefix     the gathered blob carries the gene before every UMI as kGenePrefix non-zero bytes (base-255 digits plus
//              one, big-endian: the collation's keys rely on names holding no 0 byte), so the runs of the collation are
//              the classes per (cell, gene, UMI) and a segment is a contiguous range of runs
//   classes    k_umi_classes: per run its UMI's place in the blob, n(u), its first group and its cell
//   neighbours two equal-length strings at Hamming distance 1 agree on their first L/2 bytes or on their last L - L/2.
//              Classes that share a first half are contiguous in the collated order; one more collate_resident over the
//              classes' UMIs with the halves swapped (k_umi_swap) makes those that share a second half contiguous.
//              k_umi_neighbours walks a class's half-sharing stretch in both directions, in either order, and keeps the
//              best candidate under the parent order (count, then bytes).  The walk is all pairs inside such a stretch:
//              a handful of classes on sequencing data, quadratic in the stretch on an adversarial input, exact always
//   roots      pointer jumping until nothing changes (k_umi_jump); a molecule's survivor by atomicMin of its classes'
//              first groups on the root's slot (k_umi_least); k_umi_mark_rule: every group but its molecule's survivor
//   counts     cell_corrected by the flag-scan-sample pattern of cell_dups
// Without gene_of no prefix is added, without correct the marks are k_umi_mark's: with neither, nothing else is launched.
//
// All kernels are wave64, one lane per element or per class, plain loads and vector stores; the only atomics are vector
// atomicMin: the argument checks' and k_umi_least's.  Everything runs on the null stream (collate_resident on its own)
// and leaves the device idle.
#include <hipcub/hipcub.hpp>

#include <mutex>

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

// ---- the UMI rule (gene_of, correct)
constexpr uint32_t kGenePrefix = 5; // base-255 digits of a uint32 gene id, each plus one: no 0 byte
constexpr uint32_t kNoClass = 0xffffffffu;

// oem_dedup_umis_rule, over the whole call: the smallest head of a group that takes part whose ref_id is not below n_txps
__global__ __launch_bounds__(kUT) void k_umi_check_genes(uint64_t ng, const uint32_t *__restrict__ order, const uint64_t *__restrict__ group_off,
                                                          const uint64_t *__restrict__ umi_off, const uint32_t *__restrict__ flags,
                                                          const uint32_t *__restrict__ ref_id, uint32_t n_txps,
                                                          unsigned long long *__restrict__ bad)
{
    const uint64_t g = tid64();
    if (g >= ng) return;
    const uint64_t p0 = group_off[g], p1 = group_off[g + 1];
    if (p1 == p0) return;
    const uint32_t h = order[p0];
    if (umi_off[(uint64_t)h + 1] == umi_off[h] || (flags && (flags[h] & kRecUnmapped))) return;
    if (ref_id[h] >= n_txps) atomicMin(bad, (unsigned long long)h);
}

// gene[g] of the groups that take part (0 where the ref_id is bad: *bad then names the smallest such head)
__global__ __launch_bounds__(kUT) void k_umi_genes(uint64_t ng, const uint64_t *__restrict__ part, const uint32_t *__restrict__ head,
                                                    const uint32_t *__restrict__ ref_id, uint64_t ref_id_stride,
                                                    const uint32_t *__restrict__ gene_of, uint32_t n_txps, uint32_t *__restrict__ gene,
                                                    unsigned long long *__restrict__ bad)
{
    const uint64_t g = tid64();
    if (g >= ng || !part[g]) return;
    const uint32_t h = head[g], t = ref_id[(uint64_t)h * ref_id_stride];
    if (t >= n_txps) {
        atomicMin(bad, (unsigned long long)h);
        gene[g] = 0u;
        return;
    }
    gene[g] = gene_of[t];
}

// the participants' genes close ranks as k_umi_part's heads do
__global__ __launch_bounds__(kUT) void k_umi_part_genes(uint64_t ng, const uint64_t *__restrict__ part, const uint64_t *__restrict__ pidx,
                                                         const uint32_t *__restrict__ gene, uint32_t *__restrict__ pgene)
{
    const uint64_t g = tid64();
    if (g >= ng || !part[g]) return;
    pgene[pidx[g]] = gene[g];
}

// poff (n_part + 1): the participants' UMI offsets in a dense blob; in place, every UMI moves behind its gene prefix
__global__ __launch_bounds__(kUT) void k_umi_prefix_offsets(uint64_t n_part, uint64_t *__restrict__ poff)
{
    const uint64_t q = tid64();
    if (q <= n_part) poff[q] += (uint64_t)kGenePrefix * q;
}

// blob[poff[q] .. poff[q + 1]) = the gene's digits, then the UMI of record phead[q]
__global__ __launch_bounds__(kUT) void k_umi_prefix_gather(uint64_t n_part, const uint32_t *__restrict__ phead, const uint32_t *__restrict__ pgene,
                                                            const uint8_t *__restrict__ umis, const uint64_t *__restrict__ umi_off,
                                                            const uint64_t *__restrict__ poff, uint8_t *__restrict__ blob)
{
    const uint64_t q = tid64();
    if (q >= n_part) return;
    uint8_t *dst = blob + poff[q];
    uint32_t v = pgene[q];
    for (int d = (int)kGenePrefix - 1; d >= 0; --d) {
        dst[d] = (uint8_t)(v % 255u + 1u);
        v /= 255u;
    }
    const uint64_t len = poff[q + 1] - poff[q] - kGenePrefix;
    const uint8_t *src = umis + umi_off[phead[q]];
    for (uint64_t i = 0; i < len; ++i) dst[kGenePrefix + i] = src[i];
}

// The class table.  Run r of the collation over the (prefixed) UMIs: where its string is in the blob and how long, n(u),
// its first (smallest) group and its cell; slen[r] is the length again for the scan, slen[n_cls] = 0.
__global__ __launch_bounds__(kUT) void k_umi_classes(uint64_t n_cls, const uint32_t *__restrict__ uorder, const uint64_t *__restrict__ run_off,
                                                      const uint64_t *__restrict__ poff, const uint32_t *__restrict__ pgroup,
                                                      const uint64_t *__restrict__ cell_cls_off, uint64_t nc, uint64_t *__restrict__ cls_off,
                                                      uint32_t *__restrict__ cls_len, uint32_t *__restrict__ cls_cnt,
                                                      uint32_t *__restrict__ cls_first, uint32_t *__restrict__ cls_cell,
                                                      uint64_t *__restrict__ slen, uint32_t *__restrict__ best)
{
    const uint64_t r = tid64();
    if (r > n_cls) return;
    if (r == n_cls) {
        slen[r] = 0;
        return;
    }
    const uint32_t q = uorder[run_off[r]];
    const uint64_t len = poff[(uint64_t)q + 1] - poff[q];
    cls_off[r] = poff[q];
    cls_len[r] = (uint32_t)len;
    cls_cnt[r] = (uint32_t)(run_off[r + 1] - run_off[r]);
    cls_first[r] = pgroup[q];
    cls_cell[r] = (uint32_t)last_at_or_before(cell_cls_off, nc, r);
    slen[r] = len;
    best[r] = kNoClass;
}

// sblob[soff[r] ..): class r's string with the halves of its UMI swapped behind the gene prefix: the last L - L/2 bytes,
// then the first L/2
__global__ __launch_bounds__(kUT) void k_umi_swap(uint64_t n_cls, const uint8_t *__restrict__ blob, const uint64_t *__restrict__ cls_off,
                                                   const uint32_t *__restrict__ cls_len, uint32_t gp, const uint64_t *__restrict__ soff,
                                                   uint8_t *__restrict__ sblob)
{
    const uint64_t r = tid64();
    if (r >= n_cls) return;
    const uint8_t *src = blob + cls_off[r];
    uint8_t *dst = sblob + soff[r];
    const uint32_t L = cls_len[r] - gp, h = L / 2;
    for (uint32_t i = 0; i < gp; ++i) dst[i] = src[i];
    for (uint32_t i = 0; i < L - h; ++i) dst[gp + i] = src[gp + h + i];
    for (uint32_t i = 0; i < h; ++i) dst[gp + (L - h) + i] = src[gp + i];
}

// One lane per position p of a sorted order of the classes (ord[p], or p itself where ord is NULL: the first collation).
// str / str_off: the strings that order sorts (the blob, or the swapped blob).  The classes of u's cell that share u's
// first `k` bytes -- the gene prefix and the half that this order puts first -- are one contiguous stretch around p:
// walk it in both directions and hold every class of u's length that differs from u in exactly one byte and has more
// groups against best[u], under the parent order: more groups first, then the smaller ORIGINAL bytes (blob / cls_off).
// walk[u] (or NULL): the classes looked at.
__global__ __launch_bounds__(kUT) void k_umi_neighbours(uint64_t n_cls, const uint32_t *__restrict__ ord, const uint8_t *__restrict__ str,
                                                         const uint64_t *__restrict__ str_off, uint32_t second, uint32_t gp,
                                                         const uint32_t *__restrict__ cls_len, const uint32_t *__restrict__ cls_cnt,
                                                         const uint32_t *__restrict__ cls_cell, const uint8_t *__restrict__ blob,
                                                         const uint64_t *__restrict__ cls_off, uint32_t *__restrict__ best,
                                                         uint32_t *__restrict__ walk)
{
    const uint64_t p = tid64();
    if (p >= n_cls) return;
    const uint32_t u = ord ? ord[p] : (uint32_t)p;
    const uint32_t lu = cls_len[u], L = lu - gp, h = L / 2, k = gp + (second ? L - h : h);
    const uint32_t nu = cls_cnt[u], cu = cls_cell[u];
    const uint8_t *su = str + str_off[u];
    uint32_t b = best[u], steps = 0;
    for (int dir = 0; dir < 2; ++dir) {
        uint64_t q = p;
        for (;;) {
            if (dir == 0) {
                if (q == 0) break;
                --q;
            } else if (++q >= n_cls)
                break;
            const uint32_t v = ord ? ord[q] : (uint32_t)q;
            const uint32_t lv = cls_len[v];
            if (cls_cell[v] != cu || lv < k) break;
            const uint8_t *sv = str + str_off[v];
            bool shares = true;
            for (uint32_t i = 0; i < k && shares; ++i) shares = su[i] == sv[i];
            if (!shares) break;
            ++steps;
            if (lv != lu || cls_cnt[v] <= nu) continue;
            uint32_t differ = 0;
            for (uint32_t i = k; i < lu; ++i) differ += su[i] != sv[i] ? 1u : 0u;
            if (differ != 1) continue;
            if (b != kNoClass) {
                if (cls_cnt[v] < cls_cnt[b]) continue;
                if (cls_cnt[v] == cls_cnt[b] && collate_name_cmp(blob + cls_off[v], lv, blob + cls_off[b], lv) >= 0) continue;
            }
            b = v;
        }
    }
    best[u] = b;
    if (walk) walk[u] = steps;
}

// root[u] = parent(u), or u itself; has[u] = 1 when u has a parent (has[n_cls] = 0, for the scan); least[u] = none
__global__ __launch_bounds__(kUT) void k_umi_parents(uint64_t n_cls, const uint32_t *__restrict__ best, uint32_t *__restrict__ root,
                                                      uint64_t *__restrict__ has, uint32_t *__restrict__ least)
{
    const uint64_t u = tid64();
    if (u > n_cls) return;
    if (u == n_cls) {
        has[u] = 0;
        return;
    }
    root[u] = best[u] == kNoClass ? (uint32_t)u : best[u];
    has[u] = best[u] == kNoClass ? 0ull : 1ull;
    least[u] = kNoClass;
}

// one round of pointer jumping: out[u] = in[in[u]]; *changed = 1 where that moved
__global__ __launch_bounds__(kUT) void k_umi_jump(uint64_t n_cls, const uint32_t *__restrict__ in, uint32_t *__restrict__ out,
                                                   uint32_t *__restrict__ changed)
{
    const uint64_t u = tid64();
    if (u >= n_cls) return;
    const uint32_t r = in[u], rr = in[r];
    out[u] = rr;
    if (rr != r) *changed = 1u;
}

// least[root]: the smallest first group of the root's classes, its molecule's survivor
__global__ __launch_bounds__(kUT) void k_umi_least(uint64_t n_cls, const uint32_t *__restrict__ root, const uint32_t *__restrict__ cls_first,
                                                    uint32_t *__restrict__ least)
{
    const uint64_t u = tid64();
    if (u < n_cls) atomicMin(&least[root[u]], cls_first[u]);
}

// k_umi_mark under correction: every participant but its molecule's survivor is a duplicate of it; corr[g] = 1 for the
// groups of a class that has a parent (corr: ng + 1, zero before)
__global__ __launch_bounds__(kUT) void k_umi_mark_rule(uint64_t n_part, const uint32_t *__restrict__ uorder, const uint64_t *__restrict__ run_off,
                                                        uint64_t n_runs, const uint32_t *__restrict__ pgroup, const uint32_t *__restrict__ root,
                                                        const uint32_t *__restrict__ least, const uint32_t *__restrict__ best,
                                                        uint64_t survivor_base, uint32_t *__restrict__ dup, uint64_t *__restrict__ keep,
                                                        uint64_t *__restrict__ survivor, uint64_t *__restrict__ corr)
{
    const uint64_t p = tid64();
    if (p >= n_part) return;
    const uint64_t r = last_at_or_before(run_off, n_runs, p);
    const uint32_t g = pgroup[uorder[p]], s = least[root[r]];
    if (best[r] != kNoClass) corr[g] = 1ull;
    if (g == s) return;
    dup[g] = 1u;
    keep[g] = 0ull;
    survivor[g] = survivor_base + s;
}

// cscan: the exclusive scan of corr.  cell_corrected[c] = the corrected groups of cell c.
__global__ __launch_bounds__(kUT) void k_umi_cell_corrected(uint64_t nc, const uint64_t *__restrict__ cell_group_off,
                                                             const uint64_t *__restrict__ cscan, uint64_t *__restrict__ cell_corrected)
{
    const uint64_t c = tid64();
    if (c < nc) cell_corrected[c] = cscan[cell_group_off[c + 1]] - cscan[cell_group_off[c]];
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

int umis_upload(const char *who, const uint8_t *umis, const uint64_t *umi_off, uint64_t n, DevBuf<uint8_t> *d_umis, DevBuf<uint64_t> *d_umi_off,
                bool validate)
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
                                               if (!validate) return;
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

namespace {

std::mutex g_rule_mu;
double g_rule_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};

// the largest of n uint32 on the device (the walks: a statistic only)
int max_u32(ScanTmp &t, const uint32_t *in, uint64_t n, uint32_t *d_out, uint64_t *out)
{
    size_t tb = 0;
    OEM_HIP(hipcub::DeviceReduce::Max(nullptr, tb, in, d_out, (int)n, nullptr));
    if (tb > t.cap || !t.p) {
        OEM_HIP(hipStreamSynchronize(nullptr));
        (void)hipFree(t.p);
        t.p = nullptr;
        t.cap = 0;
        OEM_HIP(hipMalloc(&t.p, tb ? tb : 1));
        t.cap = tb ? tb : 1;
    }
    tb = t.cap;
    OEM_HIP(hipcub::DeviceReduce::Max(t.p, tb, in, d_out, (int)n, nullptr));
    uint32_t v = 0;
    OEM_HIP(hipMemcpy(&v, d_out, sizeof v, hipMemcpyDeviceToHost));
    *out = v;
    return OEM_OK;
}

} // namespace

void dedup_rule_last_call(double *out8)
{
    std::lock_guard<std::mutex> lk(g_rule_mu);
    std::memcpy(out8, g_rule_last, sizeof g_rule_last);
}

void dedup_rule_reset_last()
{
    std::lock_guard<std::mutex> lk(g_rule_mu);
    std::memset(g_rule_last, 0, sizeof g_rule_last);
}

int dedup_mark(const UmiInput &in, const uint32_t *d_order, const uint32_t *d_order_bc, const uint64_t *d_group_off, uint64_t ng,
               const uint64_t *d_cell_group_off, uint32_t nc, uint64_t survivor_base, UmiMarks *out, uint64_t *cell_dups,
               uint64_t *cell_corrected)
{
    std::fill(cell_dups, cell_dups + nc, 0ull);
    if (cell_corrected) std::fill(cell_corrected, cell_corrected + nc, 0ull);
    out->n_part = out->n_classes = out->n_dups = 0;
    out->n_corrected_classes = out->jump_rounds = out->walk_max[0] = out->walk_max[1] = 0;
    out->bad_ref_record = kCollateNoRecord;
    if (!ng) return OEM_OK;
    const bool genes = in.d_gene_of != nullptr, correct = in.correct != 0;
    const uint32_t gp = genes ? kGenePrefix : 0u;
    ScanTmp tmp;
    DevBuf<uint32_t> d_head, d_phead, d_pgroup, d_gene, d_pgene;
    DevBuf<uint64_t> d_part, d_pidx, d_pcell, d_poff, d_cell_dups;
    DevBuf<uint8_t> d_blob;
    DevBuf<unsigned long long> d_bad;
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
    if (genes) { // gene(g) of the participants; a head whose ref_id is not a transcript ends the call
        OEM_TRY(dev_alloc(&d_gene.p, ng, nullptr));
        OEM_TRY(dev_alloc(&d_bad.p, 1, nullptr));
        const unsigned long long none = kNoRecord;
        OEM_HIP(hipMemcpy(d_bad.p, &none, sizeof none, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_umi_genes, grid_for(ng), dim3(kUT), 0, nullptr, ng, (const uint64_t *)d_part.p, (const uint32_t *)d_head.p,
                           in.d_ref_id, in.ref_id_stride, in.d_gene_of, in.n_txps, d_gene.p, d_bad.p);
        OEM_HIP(hipGetLastError());
        unsigned long long bad = kNoRecord;
        OEM_HIP(hipMemcpy(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost));
        if (bad != kNoRecord) {
            uint32_t t = 0;
            OEM_HIP(hipMemcpy(&t, in.d_ref_id + bad * in.ref_id_stride, sizeof t, hipMemcpyDeviceToHost));
            if (in.defer_bad_ref) {
                out->bad_ref_record = bad;
                out->bad_ref_id = t;
                return OEM_OK;
            }
            return fail(OEM_ERR_ARG, "%s: record %llu: ref_id %u is not below n_txps = %u (the head of a read that takes part in the UMI rule)",
                        in.who, bad, t, in.n_txps);
        }
    }
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
    if (genes) {
        OEM_TRY(dev_alloc(&d_pgene.p, n_part, nullptr));
        hipLaunchKernelGGL(k_umi_part_genes, grid_for(ng), dim3(kUT), 0, nullptr, ng, (const uint64_t *)d_part.p, (const uint64_t *)d_pidx.p,
                           (const uint32_t *)d_gene.p, d_pgene.p);
        OEM_HIP(hipGetLastError());
    }
    OEM_TRY(gather_name_offsets(d_phead.p, n_part, in.d_umi_off, d_poff.p));
    if (genes) {
        hipLaunchKernelGGL(k_umi_prefix_offsets, grid_for(n_part + 1), dim3(kUT), 0, nullptr, n_part, d_poff.p);
        OEM_HIP(hipGetLastError());
    }
    uint64_t nb = 0;
    OEM_HIP(hipMemcpy(&nb, d_poff.p + n_part, sizeof nb, hipMemcpyDeviceToHost));
    d_head.reset();
    d_part.reset();
    d_pidx.reset();
    d_gene.reset();
    OEM_TRY(dev_alloc(&d_blob.p, nb + 16, nullptr));
    if (genes) { // every UMI behind its gene's digits
        OEM_HIP(hipMemset(d_blob.p + nb, 0, 16));
        hipLaunchKernelGGL(k_umi_prefix_gather, grid_for(n_part), dim3(kUT), 0, nullptr, n_part, (const uint32_t *)d_phead.p,
                           (const uint32_t *)d_pgene.p, in.d_umis, in.d_umi_off, (const uint64_t *)d_poff.p, d_blob.p);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipStreamSynchronize(nullptr));
        d_pgene.reset();
    } else
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
    const uint64_t n_cls = ucr.n_groups;
    out->n_classes = n_cls;
    out->n_dups = n_part - n_cls;

    // the correction: parents among the classes, roots, the molecules' survivors
    DevBuf<uint32_t> d_best, d_root, d_least;
    if (correct && n_cls >= 2) {
        DevBuf<uint64_t> d_cls_off, d_slen, d_soff, d_has, d_hscan;
        DevBuf<uint32_t> d_cls_len, d_cls_cnt, d_cls_first, d_cls_cell, d_walk, d_root2, d_word;
        DevBuf<uint8_t> d_sblob;
        OEM_TRY(dev_alloc(&d_cls_off.p, n_cls, nullptr));
        OEM_TRY(dev_alloc(&d_cls_len.p, n_cls, nullptr));
        OEM_TRY(dev_alloc(&d_cls_cnt.p, n_cls, nullptr));
        OEM_TRY(dev_alloc(&d_cls_first.p, n_cls, nullptr));
        OEM_TRY(dev_alloc(&d_cls_cell.p, n_cls, nullptr));
        OEM_TRY(dev_alloc(&d_slen.p, n_cls + 1, nullptr));
        OEM_TRY(dev_alloc(&d_soff.p, n_cls + 1, nullptr));
        OEM_TRY(dev_alloc(&d_best.p, n_cls, nullptr));
        OEM_TRY(dev_alloc(&d_walk.p, n_cls, nullptr));
        OEM_TRY(dev_alloc(&d_word.p, 1, nullptr));
        hipLaunchKernelGGL(k_umi_classes, grid_for(n_cls + 1), dim3(kUT), 0, nullptr, n_cls, (const uint32_t *)ucr.order.p,
                           (const uint64_t *)ucr.group_off.p, (const uint64_t *)d_poff.p, (const uint32_t *)d_pgroup.p,
                           (const uint64_t *)ucr.cell_group_off.p, (uint64_t)nc, d_cls_off.p, d_cls_len.p, d_cls_cnt.p, d_cls_first.p,
                           d_cls_cell.p, d_slen.p, d_best.p);
        OEM_HIP(hipGetLastError());
        // classes that share the first half of their UMI are contiguous already
        hipLaunchKernelGGL(k_umi_neighbours, grid_for(n_cls), dim3(kUT), 0, nullptr, n_cls, (const uint32_t *)nullptr,
                           (const uint8_t *)d_blob.p, (const uint64_t *)d_cls_off.p, 0u, gp, (const uint32_t *)d_cls_len.p,
                           (const uint32_t *)d_cls_cnt.p, (const uint32_t *)d_cls_cell.p, (const uint8_t *)d_blob.p,
                           (const uint64_t *)d_cls_off.p, d_best.p, d_walk.p);
        OEM_HIP(hipGetLastError());
        OEM_TRY(max_u32(tmp, d_walk.p, n_cls, d_word.p, &out->walk_max[0]));
        // ... and those that share the second half are after one more collation, of the classes with the halves swapped
        OEM_TRY(exclusive_sum(tmp, d_slen.p, d_soff.p, n_cls + 1));
        uint64_t sb = 0;
        OEM_HIP(hipMemcpy(&sb, d_soff.p + n_cls, sizeof sb, hipMemcpyDeviceToHost));
        d_slen.reset();
        OEM_TRY(dev_alloc(&d_sblob.p, sb + 16, nullptr));
        OEM_HIP(hipMemset(d_sblob.p + sb, 0, 16));
        hipLaunchKernelGGL(k_umi_swap, grid_for(n_cls), dim3(kUT), 0, nullptr, n_cls, (const uint8_t *)d_blob.p, (const uint64_t *)d_cls_off.p,
                           (const uint32_t *)d_cls_len.p, gp, (const uint64_t *)d_soff.p, d_sblob.p);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipStreamSynchronize(nullptr));
        std::vector<uint64_t> ccell((size_t)nc + 1);
        OEM_HIP(hipMemcpy(ccell.data(), ucr.cell_group_off.p, sizeof(uint64_t) * ((size_t)nc + 1), hipMemcpyDeviceToHost));
        CollateInput c2 = cc;
        c2.cell_rec_off = ccell.data();
        c2.d_names = d_sblob.p;
        c2.d_name_off = d_soff.p;
        c2.d_n_bytes = sb;
        CollateResident scr;
        OEM_TRY(collate_resident(c2, 0, nc, 0, 0, 0, info, &scr));
        if (scr.n_groups != n_cls) return fail(OEM_ERR_STATE, "%s: the swapped UMIs of %llu classes fell into %llu runs", in.who,
                                               (unsigned long long)n_cls, (unsigned long long)scr.n_groups);
        hipLaunchKernelGGL(k_umi_neighbours, grid_for(n_cls), dim3(kUT), 0, nullptr, n_cls, (const uint32_t *)scr.order.p,
                           (const uint8_t *)d_sblob.p, (const uint64_t *)d_soff.p, 1u, gp, (const uint32_t *)d_cls_len.p,
                           (const uint32_t *)d_cls_cnt.p, (const uint32_t *)d_cls_cell.p, (const uint8_t *)d_blob.p,
                           (const uint64_t *)d_cls_off.p, d_best.p, d_walk.p);
        OEM_HIP(hipGetLastError());
        OEM_TRY(max_u32(tmp, d_walk.p, n_cls, d_word.p, &out->walk_max[1]));
        scr.order.reset();
        scr.group_off.reset();
        scr.cell_group_off.reset();
        d_sblob.reset();
        d_soff.reset();
        // the parents, how many classes have one, and the roots by pointer jumping
        OEM_TRY(dev_alloc(&d_root.p, n_cls, nullptr));
        OEM_TRY(dev_alloc(&d_root2.p, n_cls, nullptr));
        OEM_TRY(dev_alloc(&d_least.p, n_cls, nullptr));
        OEM_TRY(dev_alloc(&d_has.p, n_cls + 1, nullptr));
        OEM_TRY(dev_alloc(&d_hscan.p, n_cls + 1, nullptr));
        hipLaunchKernelGGL(k_umi_parents, grid_for(n_cls + 1), dim3(kUT), 0, nullptr, n_cls, (const uint32_t *)d_best.p, d_root.p, d_has.p,
                           d_least.p);
        OEM_HIP(hipGetLastError());
        OEM_TRY(exclusive_sum(tmp, d_has.p, d_hscan.p, n_cls + 1));
        OEM_HIP(hipMemcpy(&out->n_corrected_classes, d_hscan.p + n_cls, sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (out->n_corrected_classes) {
            for (uint32_t changed = 1; changed;) {
                changed = 0;
                OEM_HIP(hipMemcpy(d_word.p, &changed, sizeof changed, hipMemcpyHostToDevice));
                hipLaunchKernelGGL(k_umi_jump, grid_for(n_cls), dim3(kUT), 0, nullptr, n_cls, (const uint32_t *)d_root.p, d_root2.p, d_word.p);
                OEM_HIP(hipGetLastError());
                OEM_HIP(hipMemcpy(&changed, d_word.p, sizeof changed, hipMemcpyDeviceToHost));
                std::swap(d_root.p, d_root2.p);
                ++out->jump_rounds;
            }
            hipLaunchKernelGGL(k_umi_least, grid_for(n_cls), dim3(kUT), 0, nullptr, n_cls, (const uint32_t *)d_root.p,
                               (const uint32_t *)d_cls_first.p, d_least.p);
            OEM_HIP(hipGetLastError());
        }
        OEM_HIP(hipStreamSynchronize(nullptr));
        std::lock_guard<std::mutex> lk(g_rule_mu);
        g_rule_last[0] += (double)n_part;
        g_rule_last[1] += (double)n_cls;
        g_rule_last[2] += (double)out->n_corrected_classes;
        g_rule_last[3] = std::max(g_rule_last[3], (double)out->jump_rounds);
        g_rule_last[4] = std::max(g_rule_last[4], (double)out->walk_max[0]);
        g_rule_last[5] = std::max(g_rule_last[5], (double)out->walk_max[1]);
        g_rule_last[6] += 1.0;
    }
    d_blob.reset();
    d_poff.reset();
    if (!out->n_dups && !out->n_corrected_classes) return OEM_OK;

    OEM_TRY(dev_alloc(&out->gscan.p, ng + 1, nullptr));
    OEM_TRY(dev_alloc(&d_cell_dups.p, nc, nullptr));
    if (out->n_corrected_classes) { // molecules of several classes: the marks, and the corrected groups' counts
        DevBuf<uint64_t> d_corr, d_cscan;
        OEM_TRY(dev_alloc(&d_corr.p, ng + 1, nullptr));
        OEM_TRY(dev_alloc(&d_cscan.p, ng + 1, nullptr));
        OEM_HIP(hipMemset(d_corr.p, 0, sizeof(uint64_t) * (ng + 1)));
        hipLaunchKernelGGL(k_umi_mark_rule, grid_for(n_part), dim3(kUT), 0, nullptr, n_part, (const uint32_t *)ucr.order.p,
                           (const uint64_t *)ucr.group_off.p, n_cls, (const uint32_t *)d_pgroup.p, (const uint32_t *)d_root.p,
                           (const uint32_t *)d_least.p, (const uint32_t *)d_best.p, survivor_base, out->dup.p, out->keep.p, out->survivor.p,
                           d_corr.p);
        OEM_HIP(hipGetLastError());
        OEM_TRY(exclusive_sum(tmp, d_corr.p, d_cscan.p, ng + 1));
        hipLaunchKernelGGL(k_umi_cell_corrected, grid_for(nc), dim3(kUT), 0, nullptr, (uint64_t)nc, d_cell_group_off,
                           (const uint64_t *)d_cscan.p, d_cell_dups.p);
        OEM_HIP(hipGetLastError());
        if (cell_corrected) OEM_HIP(hipMemcpy(cell_corrected, d_cell_dups.p, sizeof(uint64_t) * nc, hipMemcpyDeviceToHost));
        else OEM_HIP(hipStreamSynchronize(nullptr));
    } else {
        hipLaunchKernelGGL(k_umi_mark, grid_for(n_part), dim3(kUT), 0, nullptr, n_part, (const uint32_t *)ucr.order.p,
                           (const uint64_t *)ucr.group_off.p, n_cls, (const uint32_t *)d_pgroup.p, survivor_base, out->dup.p, out->keep.p,
                           out->survivor.p);
        OEM_HIP(hipGetLastError());
    }
    OEM_TRY(exclusive_sum(tmp, out->keep.p, out->gscan.p, ng + 1));
    hipLaunchKernelGGL(k_umi_cell_dups, grid_for(nc), dim3(kUT), 0, nullptr, (uint64_t)nc, d_cell_group_off, (const uint64_t *)out->gscan.p,
                       d_cell_dups.p);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipMemcpy(cell_dups, d_cell_dups.p, sizeof(uint64_t) * nc, hipMemcpyDeviceToHost));
    if (out->n_corrected_classes) { // every class with a parent is at least one more duplicate
        out->n_dups = 0;
        for (uint32_t c = 0; c < nc; ++c) out->n_dups += cell_dups[c];
    }
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

// The body of oem_dedup_umis and, with a rule, of oem_dedup_umis_rule.
static int dedup_umis_call(const char *who, const oem_umi_rule *rule, const uint8_t *umis, const uint64_t *umi_off, const uint32_t *flags,
                           const uint32_t *ref_id, uint64_t n_records, const uint32_t *order, uint64_t n_positions,
                           const uint64_t *group_off, uint64_t n_groups, const uint64_t *cell_group_off, uint32_t n_cells, int device,
                           uint8_t *out_dup, uint64_t *out_survivor, uint64_t *out_cell_dups, uint64_t *out_cell_corrected)
{
    if (!umi_off || !group_off || !cell_group_off || !out_dup || !out_survivor || !out_cell_dups)
        return fail(OEM_ERR_ARG, "%s: umi_off, group_off, cell_group_off or an output is NULL", who);
    const uint32_t *gene_of = rule ? rule->gene_of : nullptr;
    if (rule) {
        if (rule->correct > 1) return fail(OEM_ERR_ARG, "%s: rule->correct = %u is neither 0 nor 1", who, rule->correct);
        if (gene_of && !rule->n_txps) return fail(OEM_ERR_ARG, "%s: rule->gene_of is given and rule->n_txps is 0", who);
        if (gene_of && !ref_id) return fail(OEM_ERR_ARG, "%s: rule->gene_of is given and ref_id is NULL", who);
    }
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
    if (out_cell_corrected) std::fill(out_cell_corrected, out_cell_corrected + n_cells, 0ull);
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
    DevBuf<uint32_t> d_ref_id, d_gene_of;
    if (gene_of) { // the heads' ref_id over the whole call first, so that the smallest bad one is named whatever the batches
        DevBuf<uint64_t> d_goff_all;
        OEM_TRY(dev_alloc(&d_ref_id.p, n_records, nullptr));
        OEM_TRY(dev_alloc(&d_gene_of.p, rule->n_txps, nullptr));
        OEM_TRY(dev_alloc(&d_goff_all.p, n_groups + 1, nullptr));
        OEM_HIP(hipMemcpy(d_ref_id.p, ref_id, sizeof(uint32_t) * n_records, hipMemcpyHostToDevice));
        OEM_HIP(hipMemcpy(d_gene_of.p, gene_of, sizeof(uint32_t) * rule->n_txps, hipMemcpyHostToDevice));
        OEM_HIP(hipMemcpy(d_goff_all.p, group_off, sizeof(uint64_t) * (n_groups + 1), hipMemcpyHostToDevice));
        OEM_HIP(hipMemcpy(d_bad.p, &none, sizeof none, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_umi_check_genes, grid_for(n_groups), dim3(kUT), 0, nullptr, n_groups, (const uint32_t *)d_order.p,
                           (const uint64_t *)d_goff_all.p, (const uint64_t *)d_umi_off.p, (const uint32_t *)d_flags.p,
                           (const uint32_t *)d_ref_id.p, rule->n_txps, d_bad.p);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipMemcpy(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost));
        if (bad != kNoRecord)
            return fail(OEM_ERR_ARG, "%s: record %llu: ref_id %u is not below n_txps = %u (the head of a read that takes part in the UMI rule)",
                        who, bad, ref_id[bad], rule->n_txps);
        in.d_ref_id = d_ref_id.p;
        in.ref_id_stride = 1;
        in.d_gene_of = d_gene_of.p;
        in.n_txps = rule->n_txps;
    }
    in.correct = rule ? rule->correct : 0u;

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
            OEM_TRY(dedup_mark(in, d_order.p + p0, nullptr, d_goff.p, ng, d_cgo.p, c1 - c0, g0, &mk, out_cell_dups + c0,
                               out_cell_corrected ? out_cell_corrected + c0 : nullptr));
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
}

extern "C" int oem_dedup_umis(const uint8_t *umis, const uint64_t *umi_off, const uint32_t *flags, uint64_t n_records, const uint32_t *order,
                              uint64_t n_positions, const uint64_t *group_off, uint64_t n_groups, const uint64_t *cell_group_off,
                              uint32_t n_cells, int device, uint8_t *out_dup, uint64_t *out_survivor, uint64_t *out_cell_dups)
{
    OEM_API_BEGIN
    return dedup_umis_call("oem_dedup_umis", nullptr, umis, umi_off, flags, nullptr, n_records, order, n_positions, group_off, n_groups,
                           cell_group_off, n_cells, device, out_dup, out_survivor, out_cell_dups, nullptr);
    OEM_API_END("oem_dedup_umis")
}

extern "C" int oem_dedup_umis_rule(const oem_umi_rule *rule, const uint8_t *umis, const uint64_t *umi_off, const uint32_t *flags,
                                   const uint32_t *ref_id, uint64_t n_records, const uint32_t *order, uint64_t n_positions,
                                   const uint64_t *group_off, uint64_t n_groups, const uint64_t *cell_group_off, uint32_t n_cells,
                                   int device, uint8_t *out_dup, uint64_t *out_survivor, uint64_t *out_cell_dups,
                                   uint64_t *out_cell_corrected)
{
    OEM_API_BEGIN
    dedup_rule_reset_last();
    return dedup_umis_call("oem_dedup_umis_rule", rule, umis, umi_off, flags, ref_id, n_records, order, n_positions, group_off, n_groups,
                           cell_group_off, n_cells, device, out_dup, out_survivor, out_cell_dups, out_cell_corrected);
    OEM_API_END("oem_dedup_umis_rule")
}
