// spdp_ladder_api.cpp -- spdp_ladder.h behind two plain C entries (host only: no context, no device work), so that the
// ladder's decisions can be compared with the oracle's restatements without a GPU

#include "spdp_ladder.h"

int spdp_ladder_plan(int unit, const int32_t range[4], const SpdpWindow* w, int mode, int recursive, int ubh,
                     int max_vmf_space, int noll, SpdpLadderPlan* out)
{
    if (!range || !w || !out || (unit != 1 && unit != 3)) return -1;
    const ladder::PlanPrm s = {mode, recursive, ubh, max_vmf_space, noll};
    const ladder::Plan p = unit == 1 ? ladder::plan<1>(range[0], range[1], range[2], range[3], *w, s)
                                     : ladder::plan<3>(range[0], range[1], range[2], range[3], *w, s);
    const bool lsp = p.kind == ladder::LINEAR_SPACE;
    *out = {p.kind, lsp ? p.n_imd : 0, lsp ? p.imd_intvl : 0, lsp ? p.recursive : 0};
    return 0;
}

int spdp_ladder_postwork(int unit, int recursive, int a0, int local, int sh, const int32_t range[4], int a_len, int b_len,
                         int n_imd, const int32_t* cpos, SpdpLadderStep* out, int cap)
{
    if (!range || !cpos || !out || n_imd < 1 || (unit != 1 && unit != 3)) return -1;
    int n = 0;
    auto put = [&](int kind, const ladder::Slab& s) {
        if (n < cap) out[n] = {kind, s.al, s.ar, s.bl, s.br, s.b_exgl, s.w};
        ++n;
    };
    auto sink = ladder::sink([&](int m, int k) { put(SPDP_STEP_RECORD, {m, m, k, k, 0, {0, 0, 0}}); },
                             [&](const ladder::Slab& s) { put(SPDP_STEP_SLAB, s); return true; },
                             [&](const ladder::Slab& s) { put(SPDP_STEP_HALF, s); });
    const ladder::Slab cur = {range[0], range[1], range[2], range[3], 0, {0, 0, 0}};
    if (unit == 1) ladder::postwork<1>(recursive, a0, local, sh, cur, a_len, b_len, n_imd, cpos, sink);
    else           ladder::postwork<3>(recursive, a0, local, sh, cur, a_len, b_len, n_imd, cpos, sink);
    return n;
}
