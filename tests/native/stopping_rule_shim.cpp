// stopping_rule_shim.cpp -- the pure layer of oarfish_amd/csrc/oem_stopping_rule.h compiled as host code, for
// tests/test_stopping_rule.py: the very functions the loop kernels call, behind a C ABI.
#include "../../oarfish_amd/csrc/oem_stopping_rule.h"

extern "C" {

// out = {niter', stop, converged, history[niter] written}
void shim_stopping_rule(uint32_t niter, double rel_diff, uint32_t max_iter, uint32_t min_iter_gate, uint32_t hist_cap,
                        double conv_thresh, uint32_t out[4])
{
    oem::EmParams p{0, max_iter, min_iter_gate, conv_thresh};
    p.hist_cap = hist_cap;
    const oem::RuleStep r = oem::stopping_rule(niter, rel_diff, p);
    out[0] = r.niter;
    out[1] = r.stop;
    out[2] = r.converged;
    out[3] = oem::history_records(niter, p);
}

double shim_rel_diff_term(double rel, double prev, double curr) { return oem::rel_diff_term(rel, prev, curr); }
}
