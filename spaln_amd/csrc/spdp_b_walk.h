// spdp_b_walk.h -- what follows the sweep of the unspliced aligner, one problem per thread: the last-row / last-column pass
// (lastB_ng, src/fwd2b1.cc:118-161; slastB_ng :951-967 in score mode) and the walk back over the per-cell codes that yields
// the records Vmf::traceback (src/vmf.cc:125-140) returns for forwardB_ng, in its order.  Plain functions of the problem's
// arrays, host and device alike: the kernels in spdp_b_forward.hip call them per thread, a CPU checker can call them too.
//
// The reference links a record to each cell's score: the origin, one record where a diagonal run starts behind a gap
// (direction NEWD, at the cell before the run), a new origin where a local path starts, the end records.  The codes keep the
// same information per cell: "the record list behind H(m, n)" below is what the cell's ptr leads to there.
#ifndef SPDP_B_WALK_H_
#define SPDP_B_WALK_H_

#include "spdp_b_dev.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPDP_B_HD __host__ __device__ inline
#else
#define SPDP_B_HD inline
#endif

#define SPDP_B_BLACK (INT32_MIN / 16 * 7)

struct ViewB {                    // one problem's arrays
    const DevProblemB* p;
    const int32_t* rowh;          // H plane of rowp: the DP's last row
    const int32_t* lastc;
    const uint8_t* trace;
    int k1;
};

SPDP_B_HD int edge_sum_b(const DevEdgeB& e, int i, int k1)
{
    if (i <= 0) return 0;
    const int far = i - (k1 > 1 ? k1 : 1);
    const int lng = far > 0 ? far : 0;
    return e.first + e.ext * (i - 1 - lng) + e.lng * lng;
}
SPDP_B_HD int edge_step_b(const DevEdgeB& e, bool first, int i, int k1) { return first ? e.first : (i > k1 ? e.lng : e.ext); }

// byte of cell (m, n) in the problem's trace
SPDP_B_HD int64_t trace_index_b(const DevProblemB& p, int m, int n)
{
    if (p.thin) {                                 // one tile of at most 16 rows, 16 lanes wide
        const int k = m - p.a_left - 1;
        int nlo = p.a_left + p.lw;
        if (nlo < p.b_left) nlo = p.b_left;
        ++nlo;
        const int t = n - nlo + k;
        return ((int64_t) (t >> 2) * 16 + k) * 4 + (t & 3);
    }
    const int row = m - p.a_left - 1, tile = row >> 6, k = row & 63;
    const int m0 = p.a_left + 1 + (tile << 6);
    int nlo = m0 - 1 + p.lw;
    if (nlo < p.b_left) nlo = p.b_left;
    ++nlo;
    const int t = n - nlo + k;
    return (int64_t) tile * p.tstride * 64 + ((int64_t) (t >> 2) * 64 + k) * 4 + (t & 3);
}
SPDP_B_HD bool in_band_b(const DevProblemB& p, int m, int n) { return n - m >= p.lw && n - m <= p.up; }
SPDP_B_HD int code_b(const ViewB& v, int m, int n) { return v.trace[trace_index_b(*v.p, m, n)]; }

enum { SPDP_B_DIR_NONE = 0, SPDP_B_DIR_DIAG = 1, SPDP_B_DIR_VERT = 2, SPDP_B_DIR_HORI = 3 };
// value and direction class of a cell of the last row or the last column (the cells lastB_ng looks at)
SPDP_B_HD void edge_cell_b(const ViewB& v, int m, int n, bool with_dir, int* val, int* dir)
{
    const DevProblemB& p = *v.p;
    *dir = SPDP_B_DIR_NONE;
    if (!in_band_b(p, m, n)) { *val = SPDP_B_BLACK; return; }
    if (m == p.a_left) { *val = n == p.b_right ? v.lastc[0] : edge_sum_b(p.top, n - p.b_left, v.k1); *dir = n == p.b_left ? SPDP_B_DIR_DIAG : SPDP_B_DIR_HORI; return; }
    if (n == p.b_left) { *val = edge_sum_b(p.left, m - p.a_left, v.k1); *dir = SPDP_B_DIR_VERT; return; }
    *val = n == p.b_right ? v.lastc[m - p.a_left] : v.rowh[n - p.b_left];
    if (with_dir) {
        const int c = code_b(v, m, n), w = c & SPDP_B_WIN;
        *dir = (c & SPDP_B_RESET) ? SPDP_B_DIR_NONE : (w == SPDP_B_FROM_DIAG ? SPDP_B_DIR_DIAG : (w <= SPDP_B_FROM_F2 ? SPDP_B_DIR_VERT : SPDP_B_DIR_HORI));
    }
}

struct RecOutB { int2* rec; int cap; int n; };
SPDP_B_HD void emit_b(RecOutB& o, int m, int n)
{
    if (o.n < o.cap) { o.rec[o.n].x = m; o.rec[o.n].y = n; }
    ++o.n;
}

// the record list behind H(m, n), appended to o.  own: the cell's own records count (false: the list its diagonal
// predecessor left it, what a local maximum links to)
SPDP_B_HD void walk_back_b(const ViewB& v, int local_l, int m, int n, bool own, RecOutB& o)
{
    const DevProblemB& p = *v.p;
    int state = SPDP_B_FROM_DIAG;                 // 0: at H, else inside that gap state
    // (a bound for safety: every pass moves one cell back or enters a gap state, which then moves)
    for (int guard = 2 * ((p.a_right - p.a_left) + (p.b_right - p.b_left)) + 8; guard-- > 0; ) {
        if (m <= p.a_left || n <= p.b_left || !in_band_b(p, m, n)) break;      // a boundary cell: its link is the origin
        const int c = code_b(v, m, n);
        if (state == SPDP_B_FROM_DIAG) {
            const int w = c & SPDP_B_WIN;
            if (w != SPDP_B_FROM_DIAG && own) { state = w; continue; }
            const int pm = m - 1, pn = n - 1;
            const bool pred_edge = pm == p.a_left || pn == p.b_left;
            const int pc = pred_edge ? 0 : code_b(v, pm, pn);
            const bool pred_diag = pred_edge ? (pm == p.a_left && pn == p.b_left) : ((pc & SPDP_B_WIN) == SPDP_B_FROM_DIAG && !(pc & SPDP_B_RESET));
            // the predecessor's score is zero: a reset cell, or a boundary cell that costs nothing
            const bool pred_zero = pred_edge ? (pm == p.a_left ? edge_sum_b(p.top, pn - p.b_left, v.k1) : edge_sum_b(p.left, pm - p.a_left, v.k1)) == 0
                                             : (pc & SPDP_B_RESET) != 0;
            const bool reset = c & SPDP_B_RESET;
            if (own && !reset) {
                if (!pred_diag) emit_b(o, pm, pn);                         // the NEWD record
                if (local_l && pred_zero) { emit_b(o, pm, pn); return; }    // a path that starts here: the new origin ends the list
            }
            own = true;
            m = pm; n = pn;
        } else if (state == SPDP_B_FROM_F || state == SPDP_B_FROM_F2) {
            const bool open = c & (state == SPDP_B_FROM_F ? SPDP_B_F_OPEN : SPDP_B_F2_OPEN);
            --m;
            if (open) state = SPDP_B_FROM_DIAG;
        } else {
            const bool open = c & (state == SPDP_B_FROM_E1 ? SPDP_B_E1_OPEN : SPDP_B_E2_OPEN);
            --n;
            if (open) state = SPDP_B_FROM_DIAG;
        }
    }
    emit_b(o, p.a_left, p.b_left);
}

// forward mode: lastB_ng, then the records; returns the score
SPDP_B_HD int finish_forward_b(const ViewB& v, int local, int best, int best_m, int best_n, RecOutB& o)
{
    const DevProblemB& p = *v.p;
    const int local_l = local && (p.flags & 1) && (p.flags & 4), local_r = local && (p.flags & 2) && (p.flags & 8);
    if (local_r) {
        emit_b(o, best_m, best_n);
        if (best <= SPDP_B_BLACK) return best;
        walk_back_b(v, local_l, best_m, best_n, false, o);
        return best;
    }
    const int r9 = p.b_right - p.a_right;
    int cm = p.a_right, cn = p.b_right;           // the cell whose list h9 carries
    int val, dir, dm = 0, dn = 0;
    edge_cell_b(v, p.a_right, p.b_right, true, &val, &dir);
    if (p.end_mode & 1) {
        int rw = p.up;
        if (p.b_right - p.a_left < rw) rw = p.b_right - p.a_left;
        if (rw > r9) {
            int gv, gd, gm = p.b_right - rw, gn = p.b_right;
            edge_cell_b(v, gm, gn, true, &gv, &gd);
            for (int r = rw - 1; r >= r9; --r) {
                int hv, hd;
                edge_cell_b(v, p.b_right - r, p.b_right, true, &hv, &hd);
                ++dm;
                gv += edge_step_b(p.endb, gd != SPDP_B_DIR_VERT, dm, v.k1);
                if (gv > hv) gd = SPDP_B_DIR_VERT;
                else { dm = 0; gv = hv; gd = hd; gm = p.b_right - r; gn = p.b_right; }
            }
            val = gv; dir = gd; cm = gm; cn = gn;
        }
    }
    if (p.end_mode & 2) {
        int rw = p.lw;
        if (p.b_left - p.a_right > rw) rw = p.b_left - p.a_right;
        if (rw < r9) {
            int gv, gd, gm = p.a_right, gn = p.a_right + rw;
            edge_cell_b(v, gm, gn, true, &gv, &gd);
            for (int r = rw + 1; r <= r9; ++r) {
                int hv = val, hd = dir, hm = cm, hn = cn;
                if (r < r9) { hm = p.a_right; hn = p.a_right + r; edge_cell_b(v, hm, hn, true, &hv, &hd); }
                ++dn;
                gv += edge_step_b(p.enda, gd != SPDP_B_DIR_HORI, dn, v.k1);
                if (gv > hv) gd = SPDP_B_DIR_VERT;                           // (VERT here too, as the reference has it)
                else { dn = 0; gv = hv; gd = hd; gm = hm; gn = hn; }
            }
            val = gv; dir = gd; cm = gm; cn = gn;
        }
    }
    emit_b(o, p.a_right, p.b_right);
    if (dn || dm) {
        if (dn) dm = 0;
        emit_b(o, p.a_right - dm, p.b_right - dn);
    }
    walk_back_b(v, local_l, cm, cn, true, o);
    return val;
}

// score mode: slastB_ng
SPDP_B_HD int finish_score_b(const ViewB& v, int local, int best)
{
    const DevProblemB& p = *v.p;
    if (local && (p.flags & 2) && (p.flags & 8)) return best;
    const int r9 = p.b_right - p.a_right;
    int mx, d;
    edge_cell_b(v, p.a_right, p.b_right, false, &mx, &d);
    if (p.end_mode & 1) {
        int rw = p.up;
        if (p.b_right - p.a_left < rw) rw = p.b_right - p.a_left;
        for (int r = rw; r > r9; --r) { int hv; edge_cell_b(v, p.b_right - r, p.b_right, false, &hv, &d); if (hv > mx) mx = hv; }
    }
    if (p.end_mode & 2) {
        int rw = p.lw;
        if (p.b_left - p.a_right > rw) rw = p.b_left - p.a_right;
        for (int r = rw; r < r9; ++r) { int hv; edge_cell_b(v, p.a_right, p.a_right + r, false, &hv, &d); if (hv > mx) mx = hv; }
    }
    return mx;
}

// ---- the cell of forwardB_ng and the thin form of the sweep -------------------------------------------------------------------
// One cell: H, F, F2 of the row above, the left neighbour's H, this row's running e1 / e2.  Ties as the reference has them: `>=`
// for a gap state opening and for the horizontal states against H, `>` for the vertical ones, order h, f, f2, e1, e2.  Returns
// the trace code; gain: the cell's score where it may be a local maximum (it gains over its diagonal predecessor and does
// not start a path of its own), else BLACK.
struct GapsB { int gop, gep, lgop, lgep; };
template <bool DAGP>
SPDP_B_HD int cell_forward_b(const GapsB& g, bool local_l, int diag, int sub, int up_h, int up_f, int up_f2, int left,
                             int& H, int& F, int& F2, int& e1, int& e2, int& gain)
{
    int code = 0;
    const int hv = diag + sub;
    int win = SPDP_B_FROM_DIAG, mx = hv;
    int v = up_h + g.gop;
    const bool fo = v >= up_f;
    F = (fo ? v : up_f) + g.gep;
    if (F > mx) { mx = F; win = SPDP_B_FROM_F; }
    if (fo) code |= SPDP_B_F_OPEN;
    if (DAGP) {
        v = up_h + g.lgop;
        const bool f2o = v >= up_f2;
        F2 = (f2o ? v : up_f2) + g.lgep;
        if (F2 > mx) { mx = F2; win = SPDP_B_FROM_F2; }
        if (f2o) code |= SPDP_B_F2_OPEN;
    }
    v = left + g.gop;
    const bool eo = v >= e1;
    e1 = (eo ? v : e1) + g.gep;
    if (e1 >= mx) { mx = e1; win = SPDP_B_FROM_E1; }
    if (eo) code |= SPDP_B_E1_OPEN;
    if (DAGP) {
        v = left + g.lgop;
        const bool e2o = v >= e2;
        e2 = (e2o ? v : e2) + g.lgep;
        if (e2 >= mx) { mx = e2; win = SPDP_B_FROM_E2; }
        if (e2o) code |= SPDP_B_E2_OPEN;
    }
    code |= win;
    gain = (win == SPDP_B_FROM_DIAG && hv > diag && !(local_l && diag == 0)) ? mx : SPDP_B_BLACK;
    if (local_l && mx <= 0) { mx = 0; code |= SPDP_B_RESET; }
    H = mx;
    return code;
}

// a thin request's single tile: lane k owns row m0 + k and is at column nlo + t - k in step t
struct ThinGeoB { int m0, rows, nlo, steps, steps4, top_hi; };
SPDP_B_HD ThinGeoB thin_geo_b(const DevProblemB& p)
{
    ThinGeoB g;
    g.m0 = p.a_left + 1;
    g.rows = p.a_right - p.a_left;
    int lo = g.m0 - 1 + p.lw;
    if (lo < p.b_left) lo = p.b_left;
    g.nlo = lo + 1;
    int nhi = g.m0 + g.rows - 1 + p.up;
    if (nhi > p.b_right) nhi = p.b_right;
    g.steps = nhi < g.nlo ? 0 : (nhi - g.nlo + 1) + g.rows - 1;
    g.steps4 = (g.steps + 3) & ~3;
    g.top_hi = p.up - (p.b_left - p.a_left);
    if (g.top_hi > p.b_right - p.b_left) g.top_hi = p.b_right - p.b_left;
    return g;
}
SPDP_B_HD int64_t thin_trace_bytes_b(const DevProblemB& p) { return (int64_t) thin_geo_b(p).steps4 * 16; }
// H of the top boundary row (initB_ng) at column n; columns the boundary does not reach, and those behind b_right, are black
SPDP_B_HD int thin_top_b(const DevProblemB& p, const ThinGeoB& g, int k1, int n)
{
    const int i = n - p.b_left;
    return (i >= 0 && i <= g.top_hi) ? edge_sum_b(p.top, i, k1) : SPDP_B_BLACK;
}

struct ThinLaneB {                                // what a lane carries from step to step
    int H, F, F2, e1, e2;                         // its last cell
    int up_h_prev;                                // H(m - 1, n - 1) of the coming step
    int best, best_m, best_n;                     // LocalR: the running maximum
};
SPDP_B_HD void thin_lane_init_b(const DevProblemB& p, const ThinGeoB& g, int k1, int k, ThinLaneB& L)
{
    L.H = L.F = L.F2 = L.e1 = L.e2 = SPDP_B_BLACK;
    L.up_h_prev = k == 0 ? thin_top_b(p, g, k1, g.nlo - 1) : SPDP_B_BLACK;
    L.best = SPDP_B_BLACK; L.best_m = p.a_left; L.best_n = p.b_left;
}
// step t of lane k: up_h / up_f / up_f2 are what lane k - 1 held one step ago (lane 0: the top boundary, thin_top_b / black),
// x / y the residues of row m and of column n; mtx has stride 32.  Returns the trace code (0 where the lane has no cell).
template <bool DAGP>
SPDP_B_HD int thin_step_b(const DevProblemB& p, const ThinGeoB& g, const GapsB& gp, int k1, bool local_l, bool local_r, const int* mtx,
                          int k, int t, int x, int y, int up_h, int up_f, int up_f2, ThinLaneB& L, int32_t* rowH, int32_t* lastcol)
{
    const int m = g.m0 + k, n = g.nlo + t - k;
    int rs = m - 1 + p.lw;
    if (rs < p.b_left) rs = p.b_left;
    ++rs;
    int re = m + p.up;
    if (re > p.b_right) re = p.b_right;
    int code = 0;
    if (k < g.rows && n >= rs && n <= re) {
        int diag = L.up_h_prev;
        if (n - 1 == p.b_left && m - 1 > p.a_left) diag = edge_sum_b(p.left, m - 1 - p.a_left, k1);
        int left = L.H;
        if (n == rs) {
            L.e1 = L.e2 = SPDP_B_BLACK;
            left = (n - 1 == p.b_left && p.b_left - m >= p.lw) ? edge_sum_b(p.left, m - p.a_left, k1) : SPDP_B_BLACK;
        }
        if (n - m + 1 > p.up) { up_h = SPDP_B_BLACK; up_f = SPDP_B_BLACK; up_f2 = SPDP_B_BLACK; }
        int gain;
        code = cell_forward_b<DAGP>(gp, local_l, diag, mtx[x * 32 + y], up_h, up_f, up_f2, left, L.H, L.F, L.F2, L.e1, L.e2, gain);
        if (local_r && gain > L.best) { L.best = gain; L.best_m = m; L.best_n = n; }
        if (n == p.b_right) lastcol[m - p.a_left] = L.H;
        if (k == g.rows - 1) rowH[n - p.b_left] = L.H;
    }
    L.up_h_prev = up_h;
    return code;
}

#endif
