// b_sweep_host.h -- one lspB_ng request of the unspliced aligner on the CPU, for the stand-alone checkers
// (tests/b_seeded_host_check.cpp, tests/b_thin_host_check.cpp).
//
// Everything but the sweep is the product's own code: the branches of lspB_ng without a DP cell and the boundary terms
// (spdp_b_host.h), what follows a sweep (spdp_b_walk.h: lastB_ng and the record walk) and the record fix-up.  Only the sweep
// itself is emulated: a request of at most 16 rows runs lane by lane and step by step the way spdp_b_sweep_thin runs it --
// sixteen lanes, the shift from lane k - 1, the closed-form top boundary for lane 0, the thin trace layout -- with the shared
// step function thin_step_b; a larger one (or any, with thin_allowed off) fills the tiled layout row by row with cell_forward_b.
#ifndef TESTS_B_SWEEP_HOST_H_
#define TESTS_B_SWEEP_HOST_H_

#include <cstring>
#include <vector>

struct int2 { int x, y; };
#include "../spaln_amd/csrc/spdp_b_host.h"
#include "../spaln_amd/csrc/spdp_b_walk.h"

namespace b_sweep_host {

enum { SERVED_WITHOUT_CELL = 0, SERVED_THIN = 1, SERVED_TILED = 2 };

// the request p (ranges and end flags) in window w: the score; its records, closed, appended to rec in lspB_ng's order.
// served: which of the three ways it went; failed: the record list exceeded its bound
inline int request(const SpdpScoring& sc, float tgapf, const SpdpProblem& p, const SpdpWindow& w, bool thin_allowed,
                   std::vector<SpdpSkl>& rec, int& served, bool& failed)
{
    int score = SPDP_NEVSEL;
    std::vector<SpdpSkl> r;
    failed = false;
    if (spdp_bh::lsp_without_cells(sc, p, w, score, r)) { served = SERVED_WITHOUT_CELL; rec.insert(rec.end(), r.begin(), r.end()); return score; }
    DevProblemB d;
    memset(&d, 0, sizeof d);
    spdp_bh::forward_terms(sc, tgapf, p, w, d);
    const int rows = p.a_right - p.a_left, cols = p.b_right - p.b_left;
    d.thin = (thin_allowed && rows <= 16) ? 1 : 0;
    d.tstride = d.thin ? 0 : (int) spdp_bh::tile_stride(p, w);
    d.rec_cap = (rows + cols) / 2 + 8;
    const int64_t tbytes = d.thin ? thin_trace_bytes_b(d) : spdp_bh::trace_bytes(p, w);
    std::vector<uint8_t> trace((size_t) tbytes, 0);
    std::vector<int32_t> rowh((size_t) cols + 1, SPDP_B_BLACK), lastc((size_t) rows + 1, SPDP_B_BLACK);
    std::vector<int> mtx(32 * 32, 0);
    for (int x = 1; x < sc.mtx_dim; ++x) for (int y = 1; y < sc.mtx_dim; ++y) mtx[x * 32 + y] = sc.mtx[x * sc.mtx_dim + y];
    const GapsB gp = {sc.gop, sc.gep, sc.lgop, sc.lgep};
    const int k1 = spdp_bh::k1_of(sc);
    const bool dagp = sc.noll == 3;
    const bool local_l = sc.local && p.a_exgl && p.b_exgl, local_r = sc.local && p.a_exgr && p.b_exgr;
    int best = SPDP_B_BLACK, best_m = p.a_left, best_n = p.b_left;
    if (d.thin) {
        served = SERVED_THIN;
        const ThinGeoB g = thin_geo_b(d);
        lastc[0] = thin_top_b(d, g, k1, p.b_right);
        ThinLaneB L[16];
        int y[16], blkY[16];
        for (int k = 0; k < 16; ++k) { thin_lane_init_b(d, g, k1, k, L[k]); y[k] = blkY[k] = 0; }
        for (int t = 0; t < g.steps4; ++t) {
            if ((t & 15) == 0)
                for (int k = 0; k < 16; ++k) { const int c = g.nlo + t + k; blkY[k] = (t < g.steps && c <= p.b_right) ? p.b[c - 1] : 0; }
            int H0[16], F0[16], F20[16], y0[16];
            for (int k = 0; k < 16; ++k) { H0[k] = L[k].H; F0[k] = L[k].F; F20[k] = L[k].F2; y0[k] = y[k]; }
            for (int k = 0; k < 16; ++k) {
                const int inH = (k == 0 && t < g.steps) ? thin_top_b(d, g, k1, g.nlo + t) : SPDP_B_BLACK;
                const int up_h = k ? H0[k - 1] : inH, up_f = k ? F0[k - 1] : SPDP_B_BLACK, up_f2 = (dagp && k) ? F20[k - 1] : SPDP_B_BLACK;
                y[k] = k ? y0[k - 1] : blkY[t & 15];
                const int x = k < g.rows ? p.a[g.m0 + k - 1] : 0;
                int code = 0;
                if (t < g.steps)
                    code = dagp ? thin_step_b<true>(d, g, gp, k1, local_l, local_r, mtx.data(), k, t, x, y[k], up_h, up_f, up_f2, L[k], rowh.data(), lastc.data())
                                : thin_step_b<false>(d, g, gp, k1, local_l, local_r, mtx.data(), k, t, x, y[k], up_h, up_f, up_f2, L[k], rowh.data(), lastc.data());
                trace[((size_t) (t >> 2) * 16 + k) * 4 + (t & 3)] = (uint8_t) code;
            }
        }
        for (int k = 0; k < 16; ++k) {
            const ThinLaneB& l = L[k];
            if (l.best > best || (l.best == best && (l.best_m < best_m || (l.best_m == best_m && l.best_n < best_n)))) { best = l.best; best_m = l.best_m; best_n = l.best_n; }
        }
    } else {
        served = SERVED_TILED;
        // the tiled layout, filled row by row (what a cell reads does not depend on the order the tiles visit the cells in)
        const int top_hi = std::min(cols, d.up - (p.b_left - p.a_left));
        std::vector<int> pH((size_t) cols + 1), pF((size_t) cols + 1, SPDP_B_BLACK), pF2((size_t) cols + 1, SPDP_B_BLACK), cH, cF, cF2;
        for (int i = 0; i <= cols; ++i) pH[i] = i <= top_hi ? edge_sum_b(d.top, i, k1) : SPDP_B_BLACK;
        lastc[0] = pH[cols];
        for (int m = p.a_left + 1; m <= p.a_right; ++m) {
            const int rs = std::max(p.b_left, m - 1 + d.lw) + 1, re = std::min(p.b_right, m + d.up);
            cH.assign((size_t) cols + 1, SPDP_B_BLACK); cF.assign((size_t) cols + 1, SPDP_B_BLACK); cF2.assign((size_t) cols + 1, SPDP_B_BLACK);
            const int left0 = (p.b_left - m >= d.lw) ? edge_sum_b(d.left, m - p.a_left, k1) : SPDP_B_BLACK;
            int e1 = SPDP_B_BLACK, e2 = SPDP_B_BLACK;
            for (int n = rs; n <= re; ++n) {
                const int i = n - p.b_left;
                const int diag = (n - 1 == p.b_left && m - 1 > p.a_left) ? edge_sum_b(d.left, m - 1 - p.a_left, k1) : pH[i - 1];
                const int left = n == rs ? (n - 1 == p.b_left ? left0 : SPDP_B_BLACK) : cH[i - 1];
                int up_h = pH[i], up_f = pF[i], up_f2 = pF2[i];
                if (n - m + 1 > d.up) up_h = up_f = up_f2 = SPDP_B_BLACK;
                int H, F = SPDP_B_BLACK, F2 = SPDP_B_BLACK, gain;
                const int sub = mtx[p.a[m - 1] * 32 + p.b[n - 1]];
                const int code = dagp ? cell_forward_b<true>(gp, local_l, diag, sub, up_h, up_f, up_f2, left, H, F, F2, e1, e2, gain)
                                      : cell_forward_b<false>(gp, local_l, diag, sub, up_h, up_f, up_f2, left, H, F, F2, e1, e2, gain);
                if (local_r && gain > best) { best = gain; best_m = m; best_n = n; }
                cH[i] = H; cF[i] = F; cF2[i] = F2;
                trace[(size_t) trace_index_b(d, m, n)] = (uint8_t) code;
                if (n == p.b_right) lastc[m - p.a_left] = H;
            }
            pH.swap(cH); pF.swap(cF); pF2.swap(cF2);
        }
        for (int i = 1; i <= cols; ++i) rowh[i] = pH[i];
    }
    ViewB v;
    v.p = &d; v.rowh = rowh.data(); v.lastc = lastc.data(); v.trace = trace.data(); v.k1 = k1;
    std::vector<int2> buf((size_t) d.rec_cap);
    RecOutB o;
    o.rec = buf.data(); o.cap = d.rec_cap; o.n = 0;
    score = finish_forward_b(v, sc.local, best, best_m, best_n, o);
    if (o.n > o.cap) { failed = true; return SPDP_NEVSEL; }
    for (int k = 0; k < o.n; ++k) r.push_back({buf[k].x, buf[k].y});
    spdp_bh::close_records(sc, p, r);
    rec.insert(rec.end(), r.begin(), r.end());
    return score;
}

}   // namespace b_sweep_host
#endif
