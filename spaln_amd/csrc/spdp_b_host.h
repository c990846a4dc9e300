// spdp_b_host.h -- the host side of one lspB_ng call of the unspliced aligner (src/fwd2b1.cc:1245-1269, 1070-1102), shared by
// its entries (spdp_b_api.cpp), the seeded walk (spdp_b_seeded_walk.h) and the stand-alone checker of the walk: PwdB's gap
// prices, the branches without a DP cell (empty ranges, the one-diagonal window) and the boundary terms of a problem that does
// go to the sweep.  Plain C++, no device code.
#ifndef SPDP_B_HOST_H_
#define SPDP_B_HOST_H_

#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>
#include "../../include/spdp.h"
#include "spdp_b_dev.h"

namespace spdp_bh {

constexpr int LARGEN = INT_MAX / 4 * 3;                 // src/aln.h:45

// PwdB::GapPenalty / GapExtPen / UnpPenalty (src/aln.h:275-287); codonk1 = LARGEN unless Noll == 3 (src/aln2.cc:114)
inline int k1_of(const SpdpScoring& sc) { return sc.noll == 3 ? sc.codonk1 : LARGEN; }
inline int gap_penalty(const SpdpScoring& sc, int i) { return !i ? 0 : (i > k1_of(sc) ? sc.lgop + i * sc.lgep : sc.gop + i * sc.gep); }
inline int gap_ext_pen(const SpdpScoring& sc, int i) { return i > k1_of(sc) ? sc.lgep : sc.gep; }
inline int unp_penalty(const SpdpScoring& sc, int d)
{
    const int unp = d * sc.gep;
    return d <= k1_of(sc) ? unp : unp + (sc.lgep - sc.gep) * (d - k1_of(sc));
}
inline int sim(const SpdpScoring& sc, int x, int y) { return (x && y) ? sc.mtx[x * sc.mtx_dim + y] : 0; }

inline DevEdgeB edge(const SpdpScoring& sc, float f) { return {(int) (gap_penalty(sc, 1) * f), (int) (sc.gep * f), (int) (sc.lgep * f)}; }

// Aln2b1::diagonalB_ng (src/fwd2b1.cc:1070-1102)
inline int diagonal_b(const SpdpScoring& sc, const SpdpProblem& p, std::vector<SpdpSkl>& rec)
{
    const bool LocalL = sc.local && p.a_exgl && p.b_exgl, LocalR = sc.local && p.a_exgr && p.b_exgr;
    int best = SPDP_NEVSEL, mL = p.a_left, mR = p.a_right, s = 0;
    const int d = p.b_left - p.a_left;
    for (int i = p.a_left; i < p.a_right; ) {
        s += sim(sc, p.a[i], p.b[i + d]);
        ++i;
        if (LocalL && s < 0) { s = 0; mL = i; }
        if (LocalR && s > best) { best = s; mR = i; }
    }
    rec.push_back({mL, mL + d});
    rec.push_back({mR, mR + d});
    return LocalR ? best : s;
}

// the branches of lspB_ng that need no DP cell.  true: served (score and records set); false: the problem goes to the sweep
inline bool lsp_without_cells(const SpdpScoring& sc, const SpdpProblem& p, const SpdpWindow& w, int& score, std::vector<SpdpSkl>& rec)
{
    const int rows = p.a_right - p.a_left, cols = p.b_right - p.b_left;
    if (!rows && !cols) { score = 0; return true; }
    if (!rows || !cols) {
        rec.push_back({p.a_left, p.b_left});
        rec.push_back({p.a_right, p.b_right});
        // (lspB_ng keeps b's left flag under the name of a's, src/fwd2b1.cc:1250)
        if (rows) score = (p.b_exgl || p.a_exgr) ? gap_ext_pen(sc, rows) : gap_penalty(sc, rows);
        else score = (p.b_exgl || p.b_exgr) ? gap_ext_pen(sc, cols) : unp_penalty(sc, cols);
        return true;
    }
    if (w.up == w.lw) { score = diagonal_b(sc, p, rec); return true; }
    if (w.width < 0) { score = SPDP_NEVSEL; return true; }
    return false;
}

// the tiled sweep's trace store: steps per tile (a multiple of 4) and bytes per problem
inline int64_t tile_stride(const SpdpProblem& p, const SpdpWindow& w)
{
    const int64_t cols = p.b_right - p.b_left;
    const int64_t span = std::min<int64_t>(cols, (int64_t) w.up - w.lw + SPDP_B_TILE) + SPDP_B_TILE - 1;
    return (span + 3) & ~(int64_t) 3;
}
inline int64_t trace_bytes(const SpdpProblem& p, const SpdpWindow& w)
{
    const int64_t rows = p.a_right - p.a_left;
    return (rows + SPDP_B_TILE - 1) / SPDP_B_TILE * tile_stride(p, w) * SPDP_B_TILE;
}

// the ranges, flags and boundary terms of a forward problem (initB_ng / lastB_ng with tgapf folded in); offsets are the caller's
inline void forward_terms(const SpdpScoring& sc, float tgapf, const SpdpProblem& p, const SpdpWindow& w, DevProblemB& d)
{
    d.a_left = p.a_left; d.a_right = p.a_right; d.b_left = p.b_left; d.b_right = p.b_right;
    d.a_len = p.a_len; d.b_len = p.b_len;
    d.lw = w.lw; d.up = w.up;
    d.flags = (p.a_exgl ? 1 : 0) | (p.a_exgr ? 2 : 0) | (p.b_exgl ? 4 : 0) | (p.b_exgr ? 8 : 0);
    d.top = edge(sc, p.a_left ? 1.f : (p.a_exgl ? 0.f : tgapf));
    d.left = edge(sc, p.b_left ? 1.f : (p.b_exgl ? 0.f : tgapf));
    const float fb = p.b_exgr ? 0.f : tgapf, fa = p.a_exgr ? 0.f : tgapf;
    d.endb = edge(sc, fb); d.enda = edge(sc, fa);
    d.end_mode = ((p.b_right == p.b_len && fb < 1) ? 1 : 0) | ((p.a_right == p.a_len && fa < 1) ? 2 : 0);
}

// trcbkalignB_ng's tail (src/fwd2b1.cc:1136-1141): a global path whose last record is not the origin gets it appended
inline void close_records(const SpdpScoring& sc, const SpdpProblem& p, std::vector<SpdpSkl>& r)
{
    if (!sc.local && !r.empty() && (r.back().m != p.a_left || r.back().n != p.b_left)) r.push_back({p.a_left, p.b_left});
}

}   // namespace spdp_bh
#endif
