// spdp_b_seeded_walk.h -- the seeded walk of the unspliced aligner: Aln2b1::globalB_ng with algmode.qck = 1 .. 3 ->
// seededB_ng -> backforth / creepback / creepfwrd / lspB_ng (ogotoh/spaln v3.0.7 src/fwd2b1.cc:1342-1560).  Plain C++ for the
// host alone; the types it shares with the other two walks (Span, Bound, Hsp, Unit, DpBackend) are spdp_walk.h's.
//
// This walk is the plain ancestor of seededS_ng / seededH_ng: no gap-filler table, no unit choice, no end extensions.  The HSPs
// of a level (the caller's list at the lowest level, else the first unit of Wilip(seqs, pwd, level)) are visited left to right;
// the stretch in front of each is, in this order, an abutting start (5' end: the HSP's corner is written), a switch of
// diagonals inside an overlap (backforth), a deeper level where the stretch still holds a word of that level, or a DP call
// (lspB_ng) after both neighbours were given back residue by residue while that costs less than Vthr / 2 (creepback,
// creepfwrd); an HSP the creeps swallow is skipped.  Every record goes to one list, in the reference's order.
#ifndef SPDP_B_SEEDED_WALK_H_
#define SPDP_B_SEEDED_WALK_H_

#include "spdp_walk.h"
#include "spdp_ladder.h"
#include "spdp_b_host.h"

namespace spdp_seed {

struct WalkB {
    const uint8_t* a = nullptr; const uint8_t* b = nullptr;
    int a_len = 0, b_len = 0;
    const SpdpScoring* sc = nullptr;
    int qck = 0, vthr = 0;
    int width[4] = {0, 0, 0, 0};                        // setwlprm(level)->width
    int tpl[4] = {0, 0, 0, 0};                          // setwlprm(level)->tpl
    int lowest_level = 0;                               // b->wllvl
    std::vector<Hsp> top_hsps;                          // b->jxt: CdsNo HSPs + the slot behind them; empty: none
    DpBackend* dp = nullptr;
    Span cur{};
    Records rec;
    bool unsupported = false;                           // an HSP search nobody could answer, or a DP call outside the sequences

    // (a position outside the sequences scores nothing: the reference's bounds can point there, see `bab` below, and what it
    // reads then is not defined)
    int sim2(int m, int n) const { return (m < 0 || m >= a_len || n < 0 || n >= b_len) ? 0 : spdp_bh::sim(*sc, a[m], b[n]); }
    void put(int m, int n) { rec.push_back({m, n}); }

    // two HSPs overlap by `ovr`: where along the overlap to change diagonals (src/fwd2b1.cc:1342-1374)
    int backforth(int ovr, const Bound& lub)
    {
        std::vector<int> bscr((size_t) ovr + 1, 0);
        int scr = 0, i = ovr, m = cur.al, n = cur.bl;
        while (--i >= 0 && --m >= lub.la && --n >= lub.lb) bscr[i] = scr += sim2(m, n);
        int maxscr = scr;
        scr = 0;
        int ii = ++i;
        m = cur.ar + i; n = cur.br + i;
        while (i++ < ovr && m++ < lub.ua && n++ < lub.ub) {
            scr += sim2(m - 1, n - 1);
            if ((bscr[i] += scr) > maxscr) { maxscr = bscr[i]; ii = i; }
        }
        SpdpSkl skl = {cur.ar + ii, cur.br + ii};
        rec.push_back(skl);
        int dr = (cur.br - cur.ar) - (cur.bl - cur.al);
        if (dr >= 0) skl.n -= dr; else skl.m -= (dr = -dr);
        rec.push_back(skl);
        return maxscr + spdp_bh::gap_penalty(*sc, dr);
    }
    // the left / right neighbour gives residues back to the gap (src/fwd2b1.cc:1376-1402)
    int creepback(int ovr, int bscr, const Bound& lub)
    {
        int dscr = 0;
        while (cur.al > lub.la && cur.bl > lub.lb && (ovr < 0 || dscr < bscr)) {
            dscr += sim2(cur.al - 1, cur.bl - 1);
            --cur.al; --cur.bl;
            if (++ovr == 0) bscr += dscr;
        }
        return dscr;
    }
    int creepfwrd(int& ovr, int bscr, const Bound& lub)
    {
        int dscr = 0;
        while (cur.ar < lub.ua && cur.br < lub.ub && (ovr < 0 || dscr < bscr)) {
            dscr += sim2(cur.ar, cur.br);
            ++cur.ar; ++cur.br;
            if (++ovr == 0) bscr += dscr;
        }
        return dscr;
    }
    int lsp()
    {
        if (cur.al < 0 || cur.al > cur.ar || cur.ar > a_len || cur.bl < 0 || cur.bl > cur.br || cur.br > b_len) { unsupported = true; return SPDP_NEVSEL; }
        SpdpWindow w;
        ladder::stripe<1>(cur.al, cur.ar, cur.bl, cur.br, sc->sh, &w);
        return dp->lsp(cur, w, rec);
    }

    // seededB_ng (src/fwd2b1.cc:1404-1529); eimode 1: 5' end, 2: 3' end, 3: internal
    int seeded(unsigned level, const int eimode, const Bound& lub)
    {
        const Span entry = cur;
        int cmode = eimode, agap = cur.ar - cur.al, bgap = cur.br - cur.bl, num = 0, scr = 0;
        std::vector<Unit> units;
        std::vector<Hsp>* jxt = nullptr;
        const bool given = (int) level == lowest_level && !top_hsps.empty();
        if (given) { jxt = &top_hsps; num = (int) top_hsps.size() - 1; }
        else {
            if (!dp->wilip((int) level, cur, units)) { unsupported = true; return SPDP_NEVSEL; }
            if (!units.empty()) { jxt = &units[0].jxt; num = units[0].num; }
        }
        const int slmt = vthr / 2;
        int backstep = width[level & 3], words = tpl[level & 3];
        if ((int) ++level < qck) { backstep = width[level & 3]; words = tpl[level & 3]; }
        Bound bab = lub;
        int k = 0;
        if (num) {
            std::vector<Hsp>& J = *jxt;
            J[num].jx = cur.ar; J[num].jy = cur.br;
            cur.a_exgr = cur.b_exgr = 0;
            agap = J[0].jx - cur.al; bgap = J[0].jy - cur.bl;
            for ( ; num--; ++k) {
                const Hsp h = J[k];
                scr += h.jscr;
                cur.ar = h.jx; cur.br = h.jy;
                bab.ua = h.jx + h.jlen; bab.ub = h.jy + h.jlen;
                if (J[k + 1].jx < bab.ua) bab.ua = J[k + 1].jx;
                if (J[k + 1].jy < bab.ub) bab.ub = J[k + 1].jy;
                bab.ua -= backstep; bab.ub -= backstep;
                int lx = h.jx + h.jlen / 2, ly = h.jy + h.jlen / 2;
                if (bab.ua < lx) bab.ua = lx;
                if (bab.ub < ly) bab.ub = ly;
                ly = h.jy + bab.ua - h.jx;
                lx = h.jx + bab.ub - h.jy;
                if (lx < bab.ua) bab.ua = ly;           // (the reference's own mix of the two coordinates)
                if (ly < bab.ub) bab.ub = lx;
                int ovr = std::min(agap, bgap);
                if (cmode == 1 && agap == 0) put(h.jx, h.jy);
                else if (cmode == 3 && ovr <= 0) scr += backforth(-ovr, bab);
                else if ((int) level < qck && ovr >= words) scr += seeded(level, cmode, bab);
                else {
                    scr -= creepback(ovr, slmt, bab);
                    scr -= creepfwrd(ovr, slmt, bab);
                    if (ovr < 0) {                      // skip this HSP
                        agap = J[k + 1].jx - cur.al; bgap = J[k + 1].jy - cur.bl;
                        continue;
                    }
                    scr += lsp();
                }
                if (unsupported) return SPDP_NEVSEL;
                cmode = 3;
                cur.al = h.jx + h.jlen; cur.bl = h.jy + h.jlen;
                cur.a_exgl = cur.b_exgl = 0;
                agap = J[k + 1].jx - cur.al; bgap = J[k + 1].jy - cur.bl;
                bab.la = cur.ar; bab.lb = cur.br;
            }
            cur.a_exgr = entry.a_exgr; cur.b_exgr = entry.b_exgr;
            cur.ar = entry.ar; cur.br = entry.br;
            bab.ua = lub.ua; bab.ub = lub.ub;
            if (eimode == 2 || ((int) level == lowest_level + 1 && eimode == 1)) cmode = 2;
        }
        const int ovr0 = std::min(agap, bgap);
        if (cmode == 2 && ovr0 == 0) put(cur.al, cur.bl);
        else if (cmode == 3 && ovr0 <= 0) scr += backforth(-ovr0, bab);
        else if ((int) level < qck && ovr0 > words) scr += seeded(level, cmode, bab);
        else {
            int ovr = ovr0;
            scr -= creepback(ovr, slmt, bab);
            scr -= creepfwrd(ovr, slmt, bab);
            scr += lsp();
        }
        cur.al = entry.al; cur.ar = entry.ar; cur.bl = entry.bl; cur.br = entry.br;
        if ((int) --level == lowest_level && given) { top_hsps[k].jx = a_len; top_hsps[k].jy = b_len; }
        cur.a_exgl = entry.a_exgl; cur.b_exgl = entry.b_exgl;
        return unsupported ? SPDP_NEVSEL : scr;
    }

    // globalB_ng's seeded branch (src/fwd2b1.cc:1531-1549): the record file starts with one dummy record, then the end
    // records of the fixed ends; returns the score.  rec: the dummy first
    int run(const Span& whole)
    {
        cur = whole;
        rec.clear();
        rec.push_back({0, 0});
        if (!cur.a_exgl) put(cur.al, cur.bl);
        if (!cur.a_exgr) put(cur.ar, cur.br);
        const Bound bab = {cur.al, cur.bl, cur.ar, cur.br};
        return seeded((unsigned) lowest_level, 1, bab);
    }
};

// what spdp_align_b_seeded reads of the seed bundle; null: fine, else the field that is wrong
inline const char* seed_params_refused_b(const SpdpSeedParams* sp, bool has_src, bool every_pair_brings_hsps)
{
    if (!sp) return "null SpdpSeedParams";
    if (sp->qck < 1 || sp->qck > 3) return "SpdpSeedParams.qck must be 1 .. 3";
    for (int l = 0; l < 4; ++l) if (sp->wl_width[l] < 0) return "SpdpSeedParams.wl_width must not be negative";
    if (sp->vthr < 0) return "SpdpSeedParams.vthr must not be negative";
    if (sp->lcl & ~31) return "SpdpSeedParams.lcl: only the end bits 1 .. 8 and 16 (local) are served";
    const SpdpWilipModel* m = sp->wilip;
    if (!m) {
        if (sp->qck > 1) return "SpdpSeedParams.wilip is needed with qck > 1 (the levels' tuple sizes come from it)";
        if (!every_pair_brings_hsps && !has_src) return "SpdpSeedParams.wilip is needed unless every pair brings its HSPs or an SpdpHspSource answers";
        return nullptr;
    }
    if (m->dvsp != 3) return "SpdpSeedParams.wilip->dvsp must be 3 (protein pairs)";
    if (m->lsg != 0) return "SpdpSeedParams.wilip->lsg must be 0 (no introns between protein pairs)";
    if (m->mtx_rows < 1 || m->mtx_rows > 32 || m->mtx_cols < 1 || m->mtx_cols > 32) return "SpdpSeedParams.wilip->mtx_rows and wilip->mtx_cols must be 1 .. 32";
    for (int l = 0; l < 3; ++l) {
        if (m->level[l].width < 1 || m->level[l].tpl < 1 || m->level[l].elem < 1) return "SpdpSeedParams.wilip->level: elem, tpl and width must be positive";
        if (m->level[l].bitpat_len < 0 || m->level[l].bitpat_len > 32) return "SpdpSeedParams.wilip->level: bitpat_len must be 0 .. 32";
    }
    return nullptr;
}

inline void bind_problem_b(WalkB& w, const SpdpScoring* sc, const SpdpSeedParams* sp, const SpdpProblem* p, const SpdpJuxt* hsps,
                           int n_hsps, int lowest_level)
{
    w.a = p->a; w.a_len = p->a_len; w.b = p->b; w.b_len = p->b_len;
    w.sc = sc; w.qck = sp->qck; w.vthr = sp->vthr;
    for (int l = 0; l < 4; ++l) { w.width[l] = sp->wl_width[l]; w.tpl[l] = (sp->wilip && l < 3) ? sp->wilip->level[l].tpl : 0; }
    w.lowest_level = lowest_level;
    w.top_hsps.clear();
    if (hsps && n_hsps > 0)
        for (int j = 0; j <= n_hsps; ++j) w.top_hsps.push_back({hsps[j].jx, hsps[j].jy, hsps[j].jlen, hsps[j].nid, hsps[j].jscr});
}

}   // namespace spdp_seed
#endif
