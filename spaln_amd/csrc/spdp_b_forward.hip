// spdp_b_forward.hip -- the unspliced aligner's DP on gfx950: forwardB_ng / initB_ng (src/fwd2b1.cc:82-293) with a per-cell
// traceback code, and scorealoneB_ng / sinitB_ng (:918-1068), int32 scores throughout.  Layout and mapping: spdp_b_dev.h.
// What follows the sweep (lastB_ng / slastB_ng, the walk back to the record list): spdp_b_walk.h, one problem per thread.
//
// One wave per problem, lane k = row m0 + k of a 64-row tile, step t = anti-diagonal: lane k is at column nlo + t - k.
// What a cell reads from the row above comes from lane k - 1 one step earlier (a DPP shift of H, F, F2 and the column's
// residue); lane 0 reads the row planes, 64 columns per load, and the tile's last lane writes them back in place behind it
// (it is at least as many columns behind lane 0 as it has rows, so it never overtakes the loads).  Cells outside the band or
// the ranges read as the reference's "black" record: NEVSEL, no direction.
#include <hip/hip_runtime.h>
#include "spdp_wave.h"
#include "spdp_b_dev.h"
#include "spdp_b_walk.h"

namespace {

constexpr int BLACK = SPDP_B_BLACK;

// SCORE: scorealoneB_ng (no trace, its own boundary and maximum rules); DAGP: Noll == 3
template <bool SCORE, bool DAGP>
__global__ __launch_bounds__(64) void spdp_b_sweep(const DevScoringB* __restrict__ scp, const DevProblemB* __restrict__ probs,
                                                    const uint8_t* __restrict__ codes, int32_t* __restrict__ rowp,
                                                    int32_t* __restrict__ lastc, uint8_t* __restrict__ trace,
                                                    DevResultB* __restrict__ res)
{
    __shared__ int mtx[32 * 32];
    const int lane = lane_id();
    for (int i = lane; i < 32 * 32; i += 64) mtx[i] = scp->mtx[i];
    const DevProblemB p = wave_uniform(probs[blockIdx.x]);
    const int gop = scp->gop, gep = scp->gep, lgop = scp->lgop, lgep = scp->lgep, k1 = scp->k1;
    const bool local = scp->local != 0;
    const bool local_l = local && (p.flags & 1) && (p.flags & 4), local_r = local && (p.flags & 2) && (p.flags & 8);
    const int cols = p.b_right - p.b_left, nrows = p.a_right - p.a_left;
    const int64_t plane = cols + 1;
    int32_t* rowH = rowp + p.row_off;
    int32_t* rowF = rowH + plane;
    int32_t* rowF2 = rowF + plane;
    int32_t* lastcol = lastc + p.col_off;
    const uint8_t* as = codes + p.a_off;
    const uint8_t* bs = codes + p.b_off;

    // ---- the top boundary row into the planes (initB_ng; sinitB_ng + the reference's row a_left in score mode)
    const int top_hi = min(cols, p.up - (p.b_left - p.a_left));              // last column offset the boundary reaches
    if (SCORE && !(p.flags & 1)) {
        // global left end of a: the score-only engine runs its recurrences along row a_left (horizontal states only)
        if (lane == 0) {
            int h = 0, e1 = BLACK, e2 = BLACK;
            rowH[0] = 0;
            for (int i = 1; i <= cols; ++i) {
                int v = BLACK;
                if (i <= top_hi) {
                    e1 = max(h + gop, e1) + gep;
                    v = e1;
                    if (DAGP) { e2 = max(h + lgop, e2) + lgep; v = max(v, e2); }
                    h = v;
                }
                rowH[i] = v;
            }
        }
        for (int i = lane; i <= cols; i += 64) { rowF[i] = BLACK; if (DAGP) rowF2[i] = BLACK; }
    } else {
        for (int i = lane; i <= cols; i += 64) {
            rowH[i] = i <= top_hi ? edge_sum_b(p.top, i, k1) : BLACK;
            rowF[i] = BLACK;
            if (DAGP) rowF2[i] = BLACK;
        }
    }
    stores_drained();
    __syncthreads();
    if (lane == 0) lastcol[0] = gld<true>(rowH + cols);

    int best = BLACK, best_m = p.a_left, best_n = p.b_left;
    const int ntiles = (nrows + SPDP_B_TILE - 1) / SPDP_B_TILE;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int m0 = p.a_left + 1 + tile * SPDP_B_TILE;
        const int rows = min(SPDP_B_TILE, p.a_right - m0 + 1);
        const int m = m0 + lane;
        const bool row_on = lane < rows;
        const int nlo = max(p.b_left, m0 - 1 + p.lw) + 1;
        const int nhi = min(p.b_right, m0 + rows - 1 + p.up);
        if (nhi < nlo) continue;
        const int steps = (nhi - nlo + 1) + rows - 1;
        const int steps4 = (steps + 3) & ~3;                                  // (<= tstride: the host sized it so)
        const int rs = max(p.b_left, m - 1 + p.lw) + 1, re = min(p.b_right, m + p.up);
        const int x = row_on ? as[m - 1] : 0;
        const int left0 = (p.b_left - m >= p.lw) ? edge_sum_b(p.left, m - p.a_left, k1) : BLACK;    // H(m, b_left)
        const int diag0 = edge_sum_b(p.left, m - 1 - p.a_left, k1);                                  // H(m - 1, b_left), rows below the top
        uint8_t* tr = SCORE ? nullptr : trace + p.trace_off + (int64_t) tile * p.tstride * 64;

        int H = BLACK, F = BLACK, F2 = BLACK, y = 0;          // this lane's last cell and its column's residue
        int e1 = BLACK, e2 = BLACK;
        int up_h_prev = lane == 0 ? gld<true>(rowH + (nlo - 1 - p.b_left)) : BLACK;       // H(m - 1, n - 1) of the coming step
        int blkH = BLACK, blkF = BLACK, blkF2 = BLACK, blkY = 0;
        unsigned pack = 0;
        for (int t = 0; t < steps4; ++t) {
            if ((t & 63) == 0) {                              // lane 0's next 64 columns of the row above
                const int c = nlo + t + lane;
                const bool ok = c <= p.b_right;
                blkH = ok ? gld<true>(rowH + (c - p.b_left)) : BLACK;
                blkF = ok ? gld<true>(rowF + (c - p.b_left)) : BLACK;
                blkF2 = (DAGP && ok) ? gld<true>(rowF2 + (c - p.b_left)) : BLACK;
                blkY = ok ? bs[c - 1] : 0;
            }
            const int sel = t & 63;
            const int inH = __builtin_amdgcn_readlane(blkH, sel), inF = __builtin_amdgcn_readlane(blkF, sel);
            const int inF2 = DAGP ? __builtin_amdgcn_readlane(blkF2, sel) : BLACK;
            const int inY = __builtin_amdgcn_readlane(blkY, sel);
            // what lane k - 1 computed one step ago is cell (m - 1, n); lane 0 takes the row above from the planes
            int up_h = wave_shr1(inH, H), up_f = wave_shr1(inF, F);
            int up_f2 = DAGP ? wave_shr1(inF2, F2) : BLACK;
            y = wave_shr1(inY, y);
            const int n = nlo + t - lane;
            const bool on = row_on && n >= rs && n <= re;
            int code = 0;
            if (on) {
                const int r = n - m;
                int diag = up_h_prev;
                if (n - 1 == p.b_left && m - 1 > p.a_left) diag = diag0;
                int left = H;
                if (n == rs) { e1 = e2 = BLACK; left = n - 1 == p.b_left ? left0 : BLACK; }
                if (r + 1 > p.up) { up_h = BLACK; up_f = BLACK; up_f2 = BLACK; }
                int hv = diag + mtx[x * 32 + y];
                int win = SPDP_B_FROM_DIAG, mx = hv;
                int v = up_h + gop;
                const bool fo = v >= up_f;
                F = (fo ? v : up_f) + gep;
                if (F > mx) { mx = F; win = SPDP_B_FROM_F; }
                if (fo) code |= SPDP_B_F_OPEN;
                if (DAGP) {
                    v = up_h + lgop;
                    const bool f2o = v >= up_f2;
                    F2 = (f2o ? v : up_f2) + lgep;
                    if (F2 > mx) { mx = F2; win = SPDP_B_FROM_F2; }
                    if (f2o) code |= SPDP_B_F2_OPEN;
                }
                v = left + gop;
                const bool eo = v >= e1;
                e1 = (eo ? v : e1) + gep;
                if (SCORE ? e1 > mx : e1 >= mx) { mx = e1; win = SPDP_B_FROM_E1; }
                if (eo) code |= SPDP_B_E1_OPEN;
                if (DAGP) {
                    v = left + lgop;
                    const bool e2o = v >= e2;
                    e2 = (e2o ? v : e2) + lgep;
                    if (SCORE ? e2 > mx : e2 >= mx) { mx = e2; win = SPDP_B_FROM_E2; }
                    if (e2o) code |= SPDP_B_E2_OPEN;
                }
                code |= win;
                if (local_r && win == SPDP_B_FROM_DIAG && mx > best) {
                    // forwardB_ng: the cell must gain over its predecessor and must not start a path of its own
                    if (SCORE || (hv > diag && !(local_l && diag == 0))) { best = mx; best_m = m; best_n = n; }
                }
                if (local_l && (SCORE ? mx < 0 : mx <= 0)) { mx = 0; code |= SPDP_B_RESET; }
                H = mx;
                if (n == p.b_right) lastcol[m - p.a_left] = H;
                if (lane == rows - 1) {
                    rowH[n - p.b_left] = H;
                    rowF[n - p.b_left] = F;
                    if (DAGP) rowF2[n - p.b_left] = F2;
                }
            }
            up_h_prev = up_h;
            if (!SCORE) {
                pack |= (unsigned) code << (8 * (t & 3));
                if ((t & 3) == 3) {
                    reinterpret_cast<unsigned*>(tr)[(int64_t) (t >> 2) * 64 + lane] = pack;
                    pack = 0;
                }
            }
        }
        stores_drained();                                     // the next tile reads this one's last row
    }

    // the running maximum of the local form: highest score, then the first cell in the reference's row-major order
    if (local_r) {
#pragma unroll
        for (int d = 32; d; d >>= 1) {
            const int ov = __shfl_xor(best, d), om = __shfl_xor(best_m, d), on_ = __shfl_xor(best_n, d);
            const bool take = ov > best || (ov == best && (om < best_m || (om == best_m && on_ < best_n)));
            if (take) { best = ov; best_m = om; best_n = on_; }
        }
    }
    if (lane == 0) {
        DevResultB r;
        r.score = best; r.best_m = best_m; r.best_n = best_n; r.n_rec = 0;
        res[blockIdx.x] = r;
    }
}

// The thin form: requests of 1 .. 16 rows, four per wave, one per 16-lane DPP row (layout: spdp_b_dev.h).  Lane k of a row
// owns DP row a_left + 1 + k of its request; the request is one tile, so the row above lane 0 is the closed-form top
// boundary and only the last row and the last column go to memory.  H, F, F2 of the row above come from lane k - 1 by
// row_shr1, which keeps `old` -- the boundary -- for lane 0 of every row.  The four rows of lanes stand at different columns:
// each loads the residues of its next 16 columns every 16th step and lane 0 picks its column's from them by a row-local
// permute (one ds_bpermute per step, no LDS traffic); the residue then travels down the lanes with the same shift.  The
// wave runs to the longest of its four requests (the host groups requests of like step counts); a lane past its own last
// step has no cell and stores nothing.  The cell itself is thin_step_b (spdp_b_walk.h), shared with the CPU checker.
template <bool DAGP>
__global__ __launch_bounds__(64) void spdp_b_sweep_thin(const DevScoringB* __restrict__ scp, const DevProblemB* __restrict__ probs, int n_probs,
                                                         const uint8_t* __restrict__ codes, int32_t* __restrict__ rowp,
                                                         int32_t* __restrict__ lastc, uint8_t* __restrict__ trace,
                                                         DevResultB* __restrict__ res)
{
    __shared__ int mtx[32 * 32];
    const int lane = lane_id();
    for (int i = lane; i < 32 * 32; i += 64) mtx[i] = scp->mtx[i];
    __syncthreads();
    const int k = lane & 15, row0 = lane & 48;
    const int idx = blockIdx.x * 4 + (lane >> 4);
    const bool active = idx < n_probs;
    const DevProblemB p = probs[active ? idx : n_probs - 1];
    const GapsB gp = {scp->gop, scp->gep, scp->lgop, scp->lgep};
    const int k1 = scp->k1;
    const bool local = scp->local != 0;
    const bool local_l = local && (p.flags & 1) && (p.flags & 4), local_r = local && (p.flags & 2) && (p.flags & 8);
    ThinGeoB g = thin_geo_b(p);
    if (!active) { g.rows = 0; g.steps = g.steps4 = 0; }
    int32_t* rowH = rowp + p.row_off;
    int32_t* lastcol = lastc + p.col_off;
    const uint8_t* as = codes + p.a_off;
    const uint8_t* bs = codes + p.b_off;
    unsigned* tr = reinterpret_cast<unsigned*>(trace + p.trace_off);
    if (active && k == 0) lastcol[0] = thin_top_b(p, g, k1, p.b_right);

    int longest = g.steps4;                                   // of the wave's four requests
    longest = max(longest, __shfl_xor(longest, 16));
    longest = max(longest, __shfl_xor(longest, 32));
    longest = __builtin_amdgcn_readfirstlane(longest);

    const int x = k < g.rows ? as[g.m0 + k - 1] : 0;
    ThinLaneB L;
    thin_lane_init_b(p, g, k1, k, L);
    int y = 0, blkY = 0;
    unsigned pack = 0;
    for (int t = 0; t < longest; ++t) {
        if ((t & 15) == 0) {                                  // this row of lanes: the residues of its next 16 columns
            const int c = g.nlo + t + k;
            blkY = (t < g.steps && c <= p.b_right) ? bs[c - 1] : 0;
        }
        const int n0 = g.nlo + t;                             // lane 0's column
        const int inH = (k == 0 && t < g.steps) ? thin_top_b(p, g, k1, n0) : BLACK;
        const int inY = __shfl(blkY, row0 | (t & 15));
        const int up_h = row_shr1(inH, L.H), up_f = row_shr1(BLACK, L.F);
        const int up_f2 = DAGP ? row_shr1(BLACK, L.F2) : BLACK;
        y = row_shr1(inY, y);
        int code = 0;
        if (t < g.steps) code = thin_step_b<DAGP>(p, g, gp, k1, local_l, local_r, mtx, k, t, x, y, up_h, up_f, up_f2, L, rowH, lastcol);
        pack |= (unsigned) code << (8 * (t & 3));
        if ((t & 3) == 3) {
            if (t < g.steps4) tr[(t >> 2) * 16 + k] = pack;
            pack = 0;
        }
    }

    // the running maximum of the local form within the row of lanes: highest score, then the first cell in row-major order
    // (every lane takes part: the four requests of a wave need not agree on LocalR)
#pragma unroll
    for (int d = 8; d; d >>= 1) {
        const int ov = __shfl_xor(L.best, d), om = __shfl_xor(L.best_m, d), on_ = __shfl_xor(L.best_n, d);
        const bool take = ov > L.best || (ov == L.best && (om < L.best_m || (om == L.best_m && on_ < L.best_n)));
        if (take) { L.best = ov; L.best_m = om; L.best_n = on_; }
    }
    if (active && k == 0) {
        DevResultB r;
        r.score = L.best; r.best_m = L.best_m; r.best_n = L.best_n; r.n_rec = 0;
        res[idx] = r;
    }
}

// lastB_ng / slastB_ng and the record list, one problem per thread
template <bool SCORE>
__global__ __launch_bounds__(64) void spdp_b_finish(const DevScoringB* __restrict__ scp, const DevProblemB* __restrict__ probs, int n,
                                                     const int32_t* __restrict__ rowp, const int32_t* __restrict__ lastc,
                                                     const uint8_t* __restrict__ trace, int2* __restrict__ recs,
                                                     DevResultB* __restrict__ res)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DevProblemB p = probs[i];
    ViewB v;
    v.p = &p; v.rowh = rowp + p.row_off; v.lastc = lastc + p.col_off; v.trace = SCORE ? nullptr : trace + p.trace_off; v.k1 = scp->k1;
    DevResultB r = res[i];
    if (SCORE) r.score = finish_score_b(v, scp->local, r.score);
    else {
        RecOutB o;
        o.rec = recs + p.rec_off; o.cap = p.rec_cap; o.n = 0;
        r.score = finish_forward_b(v, scp->local, r.score, r.best_m, r.best_n, o);
        r.n_rec = o.n;
    }
    res[i] = r;
}

}   // namespace

// launches both kernels of one chunk on `s`; all pointers device memory
hipError_t spdp_b_launch(hipStream_t s, bool score, bool dagp, int n, const DevScoringB* sc, const DevProblemB* probs, const uint8_t* codes,
                         int32_t* rowp, int32_t* lastc, uint8_t* trace, int2* recs, DevResultB* res)
{
    if (n <= 0) return hipSuccess;
    const dim3 g(n), b(64);
    if (score) {
        if (dagp) hipLaunchKernelGGL((spdp_b_sweep<true, true>), g, b, 0, s, sc, probs, codes, rowp, lastc, trace, res);
        else hipLaunchKernelGGL((spdp_b_sweep<true, false>), g, b, 0, s, sc, probs, codes, rowp, lastc, trace, res);
        hipLaunchKernelGGL((spdp_b_finish<true>), dim3((n + 63) / 64), b, 0, s, sc, probs, n, rowp, lastc, trace, recs, res);
    } else {
        if (dagp) hipLaunchKernelGGL((spdp_b_sweep<false, true>), g, b, 0, s, sc, probs, codes, rowp, lastc, trace, res);
        else hipLaunchKernelGGL((spdp_b_sweep<false, false>), g, b, 0, s, sc, probs, codes, rowp, lastc, trace, res);
        hipLaunchKernelGGL((spdp_b_finish<false>), dim3((n + 63) / 64), b, 0, s, sc, probs, n, rowp, lastc, trace, recs, res);
    }
    return hipGetLastError();
}

// one round of forward requests on resident codes: probs[0 .. n_wide) through the tiled sweep, probs[n_wide .. n_wide + n_thin)
// through the thin one (four per wave, in the order given), then the record walk over all of them
hipError_t spdp_b_launch_round(hipStream_t s, bool dagp, int n_wide, int n_thin, const DevScoringB* sc, const DevProblemB* probs,
                               const uint8_t* codes, int32_t* rowp, int32_t* lastc, uint8_t* trace, int2* recs, DevResultB* res)
{
    const int n = n_wide + n_thin;
    if (n <= 0) return hipSuccess;
    const dim3 b(64);
    if (n_wide > 0) {
        if (dagp) hipLaunchKernelGGL((spdp_b_sweep<false, true>), dim3(n_wide), b, 0, s, sc, probs, codes, rowp, lastc, trace, res);
        else hipLaunchKernelGGL((spdp_b_sweep<false, false>), dim3(n_wide), b, 0, s, sc, probs, codes, rowp, lastc, trace, res);
    }
    if (n_thin > 0) {
        const dim3 g((n_thin + 3) / 4);
        if (dagp) hipLaunchKernelGGL((spdp_b_sweep_thin<true>), g, b, 0, s, sc, probs + n_wide, n_thin, codes, rowp, lastc, trace, res + n_wide);
        else hipLaunchKernelGGL((spdp_b_sweep_thin<false>), g, b, 0, s, sc, probs + n_wide, n_thin, codes, rowp, lastc, trace, res + n_wide);
    }
    hipLaunchKernelGGL((spdp_b_finish<false>), dim3((n + 63) / 64), b, 0, s, sc, probs, n, rowp, lastc, trace, recs, res);
    return hipGetLastError();
}
