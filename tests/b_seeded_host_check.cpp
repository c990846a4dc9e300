// b_seeded_host_check.cpp -- the seeded walk of the unspliced aligner on the CPU, as a program of its own
// (tests/test_b_seeded_host.py builds it with -fsanitize=address,undefined and runs it on a text dump of the fixtures).
//
// It compiles the product's own headers: the walk (spdp_b_seeded_walk.h), the HSP search (spdp_hsp_host.h), the branches of
// lspB_ng without a DP cell (spdp_b_host.h) and what follows a sweep (spdp_b_walk.h: lastB_ng and the record walk).  Only the
// sweep itself is emulated: a request of at most 16 rows runs lane by lane and step by step the way spdp_b_sweep_thin runs it
// -- sixteen lanes, the shift from lane k - 1, the closed-form top boundary for lane 0, the thin trace layout -- with the
// shared step function thin_step_b; a larger one fills the tiled layout row by row with cell_forward_b.
//
// Input (whitespace-separated integers unless said): the model -- 3 levels x {elem tpl mask width gain gain1 thr xdrp cutoff
// vthr bitpat_len, 32 x bitpat, 32 x convtab}, mtx_rows mtx_cols and rows x cols entries, dvsp end_bonus crs lsg mlt
// shortquery min_hit met ser ser2 -- then mtx_dim and mtx_dim^2 entries, gop gep lgop lgep codonk1 sh, the number of cases and
// per case: id, a_len, b_len, the codes of a and of b, noll local tgapf(float) qck vthr, four end flags, four widths.
// Output per case: id, score, number of records, the records (without the dummy); a last line with counts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct int2 { int x, y; };
#include "../spaln_amd/csrc/spdp_b_seeded_walk.h"
#include "../spaln_amd/csrc/spdp_hsp_host.h"
#include "../spaln_amd/csrc/spdp_b_walk.h"

namespace {
using namespace spdp_seed;

int rd(FILE* f)
{
    int v;
    if (fscanf(f, "%d", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

struct HostBackendB : DpBackend {
    const SpdpWilipModel* wm = nullptr; const SpdpProblem* prob = nullptr; const SpdpScoring* sc = nullptr; float tgapf = 1.f;
    long n_thin = 0, n_wide = 0, n_host = 0, n_wilip = 0;
    bool failed = false;

    int lsp(const Span& s, const SpdpWindow& w, Records& rec) override
    {
        SpdpProblem p = *prob;
        p.a_left = s.al; p.a_right = s.ar; p.b_left = s.bl; p.b_right = s.br;
        p.a_exgl = s.a_exgl; p.a_exgr = s.a_exgr; p.b_exgl = s.b_exgl; p.b_exgr = s.b_exgr;
        int score = SPDP_NEVSEL;
        Records r;
        if (spdp_bh::lsp_without_cells(*sc, p, w, score, r)) { ++n_host; rec.insert(rec.end(), r.begin(), r.end()); return score; }
        DevProblemB d;
        memset(&d, 0, sizeof d);
        spdp_bh::forward_terms(*sc, tgapf, p, w, d);
        const int rows = p.a_right - p.a_left, cols = p.b_right - p.b_left;
        d.thin = rows <= 16 ? 1 : 0;
        d.tstride = d.thin ? 0 : (int) spdp_bh::tile_stride(p, w);
        d.rec_cap = (rows + cols) / 2 + 8;
        const int64_t tbytes = d.thin ? thin_trace_bytes_b(d) : spdp_bh::trace_bytes(p, w);
        std::vector<uint8_t> trace((size_t) tbytes, 0);
        std::vector<int32_t> rowh((size_t) cols + 1, SPDP_B_BLACK), lastc((size_t) rows + 1, SPDP_B_BLACK);
        std::vector<int> mtx(32 * 32, 0);
        for (int x = 1; x < sc->mtx_dim; ++x) for (int y = 1; y < sc->mtx_dim; ++y) mtx[x * 32 + y] = sc->mtx[x * sc->mtx_dim + y];
        const GapsB gp = {sc->gop, sc->gep, sc->lgop, sc->lgep};
        const int k1 = spdp_bh::k1_of(*sc);
        const bool dagp = sc->noll == 3;
        const bool local_l = sc->local && p.a_exgl && p.b_exgl, local_r = sc->local && p.a_exgr && p.b_exgr;
        int best = SPDP_B_BLACK, best_m = p.a_left, best_n = p.b_left;
        if (d.thin) {
            ++n_thin;
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
            ++n_wide;
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
        score = finish_forward_b(v, sc->local, best, best_m, best_n, o);
        if (o.n > o.cap) { failed = true; return SPDP_NEVSEL; }
        for (int k = 0; k < o.n; ++k) r.push_back({buf[k].x, buf[k].y});
        spdp_bh::close_records(*sc, p, r);
        rec.insert(rec.end(), r.begin(), r.end());
        return score;
    }
    int trcbk(const Span&, const SpdpWindow&, bool, const int*, Records&) override { failed = true; return SPDP_NEVSEL; }
    bool wilip(int level, const Span& s, std::vector<Unit>& units) override
    {
        ++n_wilip;
        const spdp_hsp::Seqs pr = {prob->a, prob->a_len, s.al, s.ar, s.a_exgl, s.a_exgr, prob->b, prob->b_len, s.bl, s.br, 1, nullptr, nullptr, nullptr};
        const spdp_hsp::GapCosts gc = {nullptr, 0, sc->gop, sc->gep, sc->lgop, sc->lgep, spdp_bh::k1_of(*sc)};
        std::vector<spdp_hsp::Unit> us;
        spdp_hsp::search(wm, pr, gc, level, us);
        std::vector<int32_t> flat;
        spdp_hsp::flatten(us, flat);
        return parse_units(flat.data(), (int32_t) flat.size(), units);
    }
};
}   // namespace

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: b_seeded_host_check cases.txt\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    static SpdpWilipModel M;
    memset(&M, 0, sizeof M);
    for (int l = 0; l < 3; ++l) {
        SpdpWilipLevel& L = M.level[l];
        L.elem = rd(f); L.tpl = rd(f); L.mask = rd(f); L.width = rd(f); L.gain = rd(f); L.gain1 = rd(f); L.thr = rd(f); L.xdrp = rd(f);
        L.cutoff = rd(f); L.vthr = rd(f); L.bitpat_len = rd(f);
        for (int i = 0; i < 32; ++i) L.bitpat[i] = (uint8_t) rd(f);
        for (int i = 0; i < 32; ++i) L.convtab[i] = (uint8_t) rd(f);
    }
    M.mtx_rows = rd(f); M.mtx_cols = rd(f);
    if (M.mtx_rows < 1 || M.mtx_rows > 32 || M.mtx_cols < 1 || M.mtx_cols > 32) return 2;
    for (int i = 0; i < M.mtx_rows * M.mtx_cols; ++i) M.mtx[i] = rd(f);
    M.dvsp = rd(f); M.end_bonus = rd(f); M.crs = rd(f); M.lsg = rd(f); M.mlt = rd(f); M.shortquery = rd(f); M.min_hit = rd(f);
    M.met = rd(f); M.ser = rd(f); M.ser2 = rd(f);
    static SpdpScoring sc0;
    memset(&sc0, 0, sizeof sc0);
    sc0.mtx_dim = rd(f);
    if (sc0.mtx_dim < 1 || sc0.mtx_dim > 32) return 2;
    for (int i = 0; i < sc0.mtx_dim * sc0.mtx_dim; ++i) sc0.mtx[i] = rd(f);
    sc0.gop = rd(f); sc0.gep = rd(f); sc0.lgop = rd(f); sc0.lgep = rd(f); sc0.codonk1 = rd(f); sc0.sh = rd(f);
    sc0.scalar_engines = 1;
    const int n_cases = rd(f);
    long n_thin = 0, n_wide = 0, n_host = 0, n_wilip = 0;
    for (int c = 0; c < n_cases; ++c) {
        const int id = rd(f), a_len = rd(f), b_len = rd(f);
        std::vector<uint8_t> a((size_t) a_len), b((size_t) b_len);
        for (int i = 0; i < a_len; ++i) a[i] = (uint8_t) rd(f);
        for (int i = 0; i < b_len; ++i) b[i] = (uint8_t) rd(f);
        SpdpScoring sc = sc0;
        sc.noll = rd(f); sc.local = rd(f);
        float tgapf;
        if (fscanf(f, "%f", &tgapf) != 1) return 2;
        SpdpSeedParams sp;
        memset(&sp, 0, sizeof sp);
        sp.qck = rd(f); sp.vthr = rd(f);
        SpdpProblem p;
        memset(&p, 0, sizeof p);
        p.a = a.data(); p.a_len = a_len; p.b = b.data(); p.b_len = b_len; p.a_right = a_len; p.b_right = b_len;
        p.a_exgl = (uint8_t) rd(f); p.a_exgr = (uint8_t) rd(f); p.b_exgl = (uint8_t) rd(f); p.b_exgr = (uint8_t) rd(f);
        for (int l = 0; l < 4; ++l) sp.wl_width[l] = rd(f);
        sp.lcl = sc.local ? 16 : 0;
        sp.wilip = &M;
        if (const char* why = seed_params_refused_b(&sp, false, false)) { fprintf(stderr, "case %d: %s\n", id, why); return 2; }
        HostBackendB be;
        be.wm = &M; be.prob = &p; be.sc = &sc; be.tgapf = tgapf;
        WalkB w;
        bind_problem_b(w, &sc, &sp, &p, nullptr, 0, 0);
        w.dp = &be;
        const Span whole = {0, a_len, 0, b_len, p.a_exgl, p.a_exgr, p.b_exgl, p.b_exgr};
        const int score = w.run(whole);
        if (be.failed || w.unsupported) { printf("%d FAILED\n", id); continue; }
        printf("%d %d %d", id, score, (int) w.rec.size() - 1);
        for (size_t k = 1; k < w.rec.size(); ++k) printf(" %d %d", w.rec[k].m, w.rec[k].n);
        printf("\n");
        n_thin += be.n_thin; n_wide += be.n_wide; n_host += be.n_host; n_wilip += be.n_wilip;
    }
    fclose(f);
    printf("# requests: %ld thin, %ld wide, %ld without a cell; %ld HSP searches\n", n_thin, n_wide, n_host, n_wilip);
    return 0;
}
