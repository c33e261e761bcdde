// oem_stopping_rule.h -- the EM loop's stopping rule and the reduction that feeds it, stated once.
//
// Reference (COMBINE-lab/oarfish v0.10.3, src/em.rs): do_em's loop `while niter < max_iter` (:181), the rel-diff
// of the two count vectors (:194-201), the early exit and the increment (:212-218); em_par repeats them (:379-405).
// Every loop driver takes its decision here: the classic sweep (oem_kernels.hip), its peer-to-peer form (oem_p2p.hip),
// the rule one pass behind (oem_tile_kernels.hip), the bootstrap's slots (oem_batch_kernels.hip), the per-cell batch
// (oem_multi_kernels.hip).  Two layers: the pure rule (host and device; nothing from HIP, so a host compiler builds it
// and tests/test_stopping_rule.py holds it to the reference at its edges), and the device helpers that apply it to a
// loop state and elect the workgroup that does.
#pragma once

#include <stdint.h>

#include "../../include/oarfish_em.h" // OEM_MIN_READ_THRESH (plain C)

#ifdef __HIPCC__
#include <hip/hip_runtime.h> // (the device layer below)
#define OEM_HD __host__ __device__
#else
#define OEM_HD
#endif

namespace oem {

// Parameters that do not change during a run.
struct EmParams {
    uint32_t n_txps;
    uint32_t max_iter;
    uint32_t min_iter_gate;
    uint32_t hist_cap; // entries of EmState / BatchState::history: min(OEM_OPT_RUN_HISTORY, max_iter); later passes are not
                       // stored.  (In the word that was padding: the kernels' argument blocks keep their layout.)
    double conv_thresh;
    EmParams(uint32_t t, uint32_t m, uint32_t g, double c) : n_txps(t), max_iter(m), min_iter_gate(g), hist_cap(0), conv_thresh(c) {}
};
static_assert(sizeof(EmParams) == 24, "EmParams layout");

// One element's share of em.rs:194-201: the SIGNED relative change of an abundance above the read threshold, folded
// into the running maximum.  `rel` starts at 0 (em.rs:169), so a negative change never wins.
OEM_HD inline double rel_diff_term(double rel, double prev, double curr)
{
    if (prev > OEM_MIN_READ_THRESH) rel = __builtin_fmax(rel, (curr - prev) / prev);
    return rel;
}

// What one iteration's rel_diff does to the loop.
struct RuleStep {
    uint32_t niter; // em.rs:170, after this iteration
    bool stop;      // the loop ends here
    bool converged; // ... through `break`
};
OEM_HD inline RuleStep stopping_rule(uint32_t niter, double rel_diff, const EmParams &p)
{
    if (rel_diff < p.conv_thresh && niter > p.min_iter_gate) return {niter, true, true}; // em.rs:212 / :399: break, niter as it is
    niter += 1;                                                                         // em.rs:218 / :405
    return {niter, niter >= p.max_iter, false};                                         // em.rs:181 loop condition
}

// OEM_OPT_RUN_HISTORY: iteration `niter` (as the rule sees it, before the increment) is stored at history[niter]
OEM_HD inline bool history_records(uint32_t niter, const EmParams &p) { return niter < p.hist_cap; }

#ifdef __HIPCC__
// The rule applied to a loop state by the one lane that decides.  State: EmState or BatchState (the words last_rel,
// n_passes, niter, converged, history), in memory or a register copy.  Returns `stop`; what stopping means to the
// caller's state machine (done, phase, the final buffer) is the caller's.
template <typename State>
__device__ __forceinline__ bool decide(State *st, double rel_diff, const EmParams &p)
{
    st->last_rel = rel_diff;
    st->n_passes += 1;
    const uint32_t niter = st->niter;
    if (st->history && history_records(niter, p)) st->history[niter] = rel_diff;
    const RuleStep r = stopping_rule(niter, rel_diff, p);
    if (r.converged) st->converged = 1;
    else st->niter = r.niter;
    return r.stop;
}

__device__ __forceinline__ double wave_max(double v)
{
    for (int off = 32; off > 0; off >>= 1) v = __builtin_fmax(v, __shfl_xor(v, off, 64));
    return v;
}

// Thread 0 of a workgroup, after its atomicMax of the workgroup's maximum: draws a ticket; true for the workgroup
// that arrives last (it resets the counter).  Non-negative doubles order like their bit patterns.  Both the maximum
// and the ticket are device-scope read-modify-write atomics, performed at the one point of coherence of their line
// (memory side), and on gfx9 a no-return atomic is counted by vmcnt until it has been performed there: draining vmcnt
// before taking the ticket means the maximum is in place before the ticket can be observed, so the workgroup that
// draws the last ticket reads (with an agent-scope atomic load) a maximum that contains every workgroup's.  A release
// fence here would add an L2 write-back (buffer_wbl2) that publishes nothing this decision needs (~3.5 us per
// workgroup tail, measured in round 1).  The election is hammered in isolation by oem_test_reldiff_stress (test-only
// library, through k_reldiff_swap_clear): > 10^5 launches over 1..64 workgroups, planted maxima, the decision
// workgroup's view compared bit for bit.
__device__ __forceinline__ bool elect_last(uint32_t *counter)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return atomicAdd(counter, 1u) == gridDim.x - 1;
}

// The threads' maxima -> the workgroup's -> atomicMax of its bit pattern into *slot (if > 0), then the election.
// Workgroup-uniform result; every thread of the kThreads must call.
template <int kThreads>
__device__ __forceinline__ bool workgroup_max_and_elect(double rel, unsigned long long *slot, uint32_t *counter)
{
    __shared__ double smax[kThreads / 64];
    __shared__ bool is_last;
    rel = wave_max(rel);
    if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = rel;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = smax[0];
        for (int i = 1; i < kThreads / 64; ++i) m = __builtin_fmax(m, smax[i]);
        if (m > 0.0) atomicMax(slot, (unsigned long long)__double_as_longlong(m));
        is_last = elect_last(counter);
    }
    __syncthreads();
    return is_last;
}
#endif // __HIPCC__

} // namespace oem
