// spdp_ladder.h -- the reference's linear-space ladder, stated once for cDNA and protein queries (host only).
//   stripe / stripe31                       src/aln2.cc:156-198
//   lspS_ng / lspH_ng up to the engine      src/fwd2s1.cc:1801-1897, src/fwd2h1.cc:2140-2180
//   mimd_postwork / rcsv_postwork           src/fwd2s1.cc:1714-1799, src/fwd2h1.cc:2045-2138
// U is the row unit: one query row spans U genomic columns (1 cDNA, 3 protein).  Everything in which the two
// ladders differ beyond that factor is a member of Unit<U>; the callers (spdp_host.cpp, spdp_h_api.cpp) keep what
// differs in substance: prices, the diagonal walk, unsupported ranges and the queues.
#ifndef SPDP_LADDER_H_
#define SPDP_LADDER_H_

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include "../../include/spdp.h"

namespace ladder {

template <int U> struct Unit;
template <> struct Unit<1> {
    static const int pad = 3;                                           // width = up - lw + pad
    static bool direct(int m, int n) { return abs(n - m) < 8 || m == 1 || n == 1; }     // straight to the traceback
    static float coef_C(int noll) { return (noll + 1) * sizeof(int); }
    static int b_exgl(int flag) { return flag ? 1 : 0; }               // cpos column 1 -> b->inex.exgl
    static const bool inside_parent = false;                            // mimd_postwork does not look at the parent's ends,
    static const bool local_whole = true;                               // and a local call that crosses nothing is traced back whole
};
template <> struct Unit<3> {
    static const int pad = 7;
    static bool direct(int m, int n) { return abs(n - m) < 16 || m == 1 || n <= 3; }
    static float coef_C(int) { return 12.f; }                           // (Noll + 1) * sizeof(int), src/fwd2h1.cc:119
    static int b_exgl(int flag) { return flag; }                        // the engines tell 1 from 2
    static const bool inside_parent = true;                             // a slab beyond the parent ends the walk
    static const bool local_whole = false;
};

template <int U>
inline void stripe(int al, int ar, int bl, int br, int sh, SpdpWindow* w)
{
    if (sh < 0) sh = -sh * std::min(ar - al, br - bl) / 100;
    sh *= U;
    w->up = br - U * ar;
    w->lw = bl - U * al;
    if (w->up < w->lw) std::swap(w->up, w->lw);
    w->up += sh;
    w->lw -= sh;
    w->up = std::min(w->up, br - U * al);
    w->lw = std::max(w->lw, bl - U * ar);
    w->width = w->up - w->lw + Unit<U>::pad;
}

// ---- what lspS_ng / lspH_ng decide before any engine runs
enum Kind { EMPTY = 0, ONE_SEQUENCE, DIAGONAL, TRACEBACK, LINEAR_SPACE };
struct Plan { int kind, n_imd, imd_intvl, recursive; };                 // the last three: LINEAR_SPACE only
struct PlanPrm { int mode, recursive, ubh, max_vmf_space, noll; };      // mode: SpdpScoring[H].scalar_engines

template <int U>
inline Plan plan(int al, int ar, int bl, int br, const SpdpWindow& w, const PlanPrm& s)
{
    const int m = ar - al, n = br - bl;
    Plan p = {TRACEBACK, 0, 0, 0};
    if (!m || !n) { p.kind = !m && !n ? EMPTY : ONE_SEQUENCE; return p; }
    if (w.up == w.lw) { p.kind = DIAGONAL; return p; }
    if (Unit<U>::direct(m, n)) return p;
    // the thresholds are compared bit for bit with the reference's: operand types and order as there
    const float coef_B = 2.f;                                           // sizeof(short)
    float cvol = float(m) * (n + U * m);                                // rhombic, simd >= 2
    if (s.mode >= 1) {                                                  // hexagonal, simd < 2
        const float k = w.lw - bl + U * ar;
        const float q = br - U * al - w.up;
        cvol = float(m) * n - (k * k + q * q) / (2 * U);
    }
    if (coef_B * cvol < s.max_vmf_space) return p;
    p.n_imd = 1;
    p.imd_intvl = (m + 1) / 2;
    p.recursive = s.recursive != 0;                                     // algmode.alg & 4 (-A4 .. -A7)
    if (!p.recursive) {
        const float coef_C = Unit<U>::coef_C(s.noll);
        const double z = 2. * m * coef_B / coef_C;
        const int imd1 = int(pow(z, 1. / 3) + 0.5) - 1;
        const float spc = coef_C * n * imd1 + coef_B * cvol / (imd1 + 1) / (imd1 + 1);
        if (spc > s.max_vmf_space) p.recursive = 1;
        else {
            const int imd3 = m / 16;                                    // rows per stripe of the reference (Nelem)
            p.n_imd = s.ubh ? s.ubh : std::min(imd1, imd3);
            p.imd_intvl = (m + p.n_imd) / (p.n_imd + 1);
            if (p.imd_intvl * p.n_imd == m) --p.n_imd;
            if (p.n_imd == 0) return p;
        }
    }
    p.kind = LINEAR_SPACE;
    return p;
}

// ---- the cpos rows of a finished linear-space call: records, slabs to trace back, halves for the next round
struct Slab { int al, ar, bl, br, b_exgl; SpdpWindow w; };              // (the other three end flags of a slab are 0)

// window of a slab: its band under SIMD; under -A0 the diagonal bounds hirschberg[SH]_ng left in columns 8 and 9
template <int U>
inline void slab_window(Slab& s, bool a0, int sh, const int32_t* row)
{
    if (!a0) { stripe<U>(s.al, s.ar, s.bl, s.br, sh, &s.w); return; }
    s.w.lw = row[8]; s.w.up = row[9];
    s.w.width = s.w.up - s.w.lw + Unit<U>::pad;
}

// The positions of a row from column c to its terminator, as records of row m; returns the terminator's column.
// Column 8 is never read as a position where it is a bound: the -A0 engines give up a call whose terminator would
// land beyond column 7 (flag -3).  The SIMD engines keep no bounds and may close a row as late as column 9.
template <class Sink>
inline int row_records(const int32_t* row, int c, int m, Sink& sink)
{
    for ( ; c < 10 && row[c] < SPDP_END_OF_ULK; ++c) sink.record(m, row[c]);
    return c;
}

// Sink: void record(int m, int n); bool slab(const Slab&) -- false ends the walk; void half(const Slab&).
template <class R, class S, class H> struct Sink { R record; S slab; H half; };
template <class R, class S, class H> inline Sink<R, S, H> sink(R r, S s, H h) { return {r, s, h}; }

// cur: the range the engine wrote back; a_len, b_len: the parent's lengths (read where Unit<U>::inside_parent).
template <int U, class Sink>
inline void postwork(bool recursive, bool a0, bool local, int sh, Slab cur, int a_len, int b_len, int n_imd,
                     const int32_t* cpos, Sink& sink)
{
    const int end = SPDP_END_OF_ULK;
    cur.b_exgl = 0;
    if (recursive) {                                                    // rcsv_postwork: two half problems
        if (cpos[0] < end) {
            const int c = row_records(cpos, 2, cpos[0], sink);
            Slab first = cur, second = cur;
            first.ar = cpos[0]; first.br = cpos[c - 1];
            slab_window<U>(first, a0, sh, cpos);
            sink.half(first);
            second.al = cpos[0]; second.b_exgl = Unit<U>::b_exgl(cpos[1]); second.bl = cpos[2];
            slab_window<U>(second, a0, sh, cpos + 10);
            sink.half(second);
        } else if (Unit<U>::local_whole && local) {
            slab_window<U>(cur, false, sh, nullptr);
            sink.slab(cur);
        }
        return;
    }
    const int aleft = cur.al, bleft = cur.bl;                           // mimd_postwork: one slab per crossed row, top down
    int i = n_imd;
    while (--i >= 0 && cpos[10 * i] == end) ;
    for ( ; i >= 0 && cpos[10 * i] != end; --i) {
        const int32_t* row = cpos + 10 * i;
        cur.al = row[0]; cur.b_exgl = Unit<U>::b_exgl(row[1]); cur.bl = row[2];
        if (Unit<U>::inside_parent && (cur.ar > a_len || cur.br > b_len || cur.al < 0 || cur.bl < 0)) return;
        if (cur.bl < 0 || cur.bl > cur.br) break;
        const int c = row_records(row, 3, cur.al, sink);
        slab_window<U>(cur, a0, sh, row + 10);
        if (!sink.slab(cur)) return;
        cur.ar = cur.al;
        cur.br = row[c - 1];
    }
    if ((i < 0 && cpos[0] != end) || cpos[2] != end) {                  // the slab above the topmost crossed row
        cur.al = aleft; cur.bl = bleft;
        slab_window<U>(cur, a0, sh, cpos);
        sink.slab(cur);
    }
}

}   // namespace ladder
#endif
