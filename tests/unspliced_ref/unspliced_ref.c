/* unspliced_ref.c -- plain-C restatement of the unspliced aligner (class Aln2b1, src/fwd2b1.cc of spaln v3.0.7) for the checker.
 * TEST INFRASTRUCTURE ONLY: scalar, one problem at a time, arrays indexed by diagonal as the reference keeps them, traceback
 * through a growing list of linked records.  What is restated, by reference line:
 *   ubr_forward        forwardB_ng :163-293 with initB_ng :82-116 and lastB_ng :118-161
 *   ubr_scorealone     scorealoneB_ng :969-1068 with sinitB_ng :918-949 and slastB_ng :951-967
 *   ubr_align          globalB_ng :1531-1560 (qck = 0) over the direct part of lspB_ng :1245-1269, diagonalB_ng :1070-1102,
 *                      trcbkalignB_ng :1104-1148, Vmf::traceback (src/vmf.cc:125-140), stdskl (src/gaps.cc:140-180)
 *   ubr_rescore        skl_rngB_ng :295-395 after trimskl (src/gaps.cc:254-273), with the Cigar / Vulgar / SAM pushes
 * The linear-space branch (hirschbergB_ng) is not restated: see include/spdp.h. */
#include <stdlib.h>
#include <string.h>
#include <limits.h>
#include "spdp.h"

#define NEVSEL SPDP_NEVSEL
#define LARGEN (INT_MAX / 4 * 3)
enum { DEAD = 0, DIAG = 2, NEWD = 3, VERT = 4, HORI = 8, HORL = 11 };   /* TraceBackDir, src/aln.h:30-35 */
static int is_diag(int d) { d &= 15; return d == 2 || d == 3; }
static int is_vert(int d) { d &= 15; return (d >= 4 && d <= 7) || d == 12; }
static int is_hori(int d) { d &= 15; return (d >= 8 && d <= 11) || d == 13; }

typedef struct { int val, ptr, dir; } Cell;
typedef struct { int m, n, p; } Link;
typedef struct { Link* r; int n, cap; } Links;

static int links_add(Links* v, int m, int n, int p)
{
    if (v->n == v->cap) { v->cap = v->cap ? 2 * v->cap : 256; v->r = (Link*) realloc(v->r, sizeof(Link) * v->cap); }
    v->r[v->n].m = m; v->r[v->n].n = n; v->r[v->n].p = p;
    return v->n++;
}

typedef struct { SpdpSkl* r; int n, cap; } Recs;
static void recs_add(Recs* v, int m, int n)
{
    if (v->n == v->cap) { v->cap = v->cap ? 2 * v->cap : 64; v->r = (SpdpSkl*) realloc(v->r, sizeof(SpdpSkl) * v->cap); }
    v->r[v->n].m = m; v->r[v->n].n = n; ++v->n;
}

/* PwdB::GapPenalty / GapExtPen / UnpPenalty, src/aln.h:275-287; codonk1 as PwdB::PwdB sets it (src/aln2.cc:114) */
static int k1_of(const SpdpScoring* sc) { return sc->noll == 3 ? sc->codonk1 : LARGEN; }
static int gap_penalty(const SpdpScoring* sc, int i)
{
    if (i == 0) return 0;
    return i > k1_of(sc) ? sc->lgop + i * sc->lgep : sc->gop + i * sc->gep;
}
static int gap_ext_pen(const SpdpScoring* sc, int i) { return i > k1_of(sc) ? sc->lgep : sc->gep; }
static int unp_penalty(const SpdpScoring* sc, int d)
{
    const int unp = d * sc->gep;
    return d <= k1_of(sc) ? unp : unp + (sc->lgep - sc->gep) * (d - k1_of(sc));
}
static int sim(const SpdpScoring* sc, int x, int y) { return (x && y) ? sc->mtx[x * sc->mtx_dim + y] : 0; }

void ubr_stripe(const SpdpProblem* p, int sh, SpdpWindow* w)        /* stripe, src/aln2.cc:156-176 */
{
    const int rows = p->a_right - p->a_left, cols = p->b_right - p->b_left;
    if (sh < 0) sh = -sh * (rows < cols ? rows : cols) / 100;
    w->up = p->b_right - p->a_right;
    w->lw = p->b_left - p->a_left;
    if (w->up < w->lw) { const int t = w->up; w->up = w->lw; w->lw = t; }
    w->up += sh; w->lw -= sh;
    if (p->b_right - p->a_left < w->up) w->up = p->b_right - p->a_left;
    if (p->b_left - p->a_right > w->lw) w->lw = p->b_left - p->a_right;
    w->width = w->up - w->lw + 3;
}

int64_t ubr_cells(const SpdpProblem* p, const SpdpWindow* w)
{
    int64_t c = 0;
    for (int m = p->a_left + 1; m <= p->a_right; ++m) {
        int lo = m - 1 + w->lw, hi = m + w->up;
        if (lo < p->b_left) lo = p->b_left;
        if (hi > p->b_right) hi = p->b_right;
        if (hi > lo) c += hi - lo;
    }
    return c;
}

/* forwardB_ng: returns the score; pp = the last link of the path (0: none) */
static int forward(const SpdpScoring* sc, const SpdpUnsplicedParams* up, const SpdpProblem* p, const SpdpWindow* w, Links* vmf, int* pp)
{
    const int dagp = sc->noll == 3;
    const int LocalL = sc->local && p->a_exgl && p->b_exgl, LocalR = sc->local && p->a_exgr && p->b_exgr;
    const int al = p->a_left, ar = p->a_right, bl = p->b_left, br = p->b_right;
    const int nol = dagp ? 3 : 2;
    Cell* buf = (Cell*) malloc(sizeof(Cell) * (size_t) nol * w->width);
    for (int i = 0; i < nol * w->width; ++i) { buf[i].val = NEVSEL; buf[i].ptr = 0; buf[i].dir = 0; }
    Cell* H = buf - w->lw + 1;
    Cell* F = H + w->width;
    Cell* F2 = F + w->width;
    int best = NEVSEL, best_m = al, best_n = bl, best_p = 0;
    links_add(vmf, 0, 0, 0);
    /* initB_ng */
    {
        const int origin = links_add(vmf, al, bl, 0);
        float f = al ? 1.f : (p->a_exgl ? 0.f : up->tgapf);
        int r = bl - al, rr = br - al;
        H[r].val = 0; H[r].dir = NEWD; H[r].ptr = origin;
        if (w->up < rr) rr = w->up;
        for (int i = 1; ++r <= rr; ++i) {
            const int gpn = i == 1 ? gap_penalty(sc, 1) : gap_ext_pen(sc, i);
            H[r].dir = HORI; H[r].ptr = origin; H[r].val = H[r - 1].val + (int) (gpn * f);
        }
        f = bl ? 1.f : (p->b_exgl ? 0.f : up->tgapf);
        r = bl - al; rr = bl - ar;
        if (w->lw > rr) rr = w->lw;
        for (int i = 1; --r >= rr; ++i) {
            const int gpn = i == 1 ? gap_penalty(sc, 1) : gap_ext_pen(sc, i);
            H[r].dir = VERT; H[r].ptr = origin; H[r].val = H[r + 1].val + (int) (gpn * f);
            F[r] = H[r];
        }
    }
    for (int m = al + 1; m <= ar; ++m) {
        Cell e1 = {NEVSEL, 0, 0}, e2 = {NEVSEL, 0, 0};
        int n = m - 1 + w->lw;
        if (n < bl) n = bl;
        int n9 = m + w->up;
        if (n9 > br) n9 = br;
        const int x = p->a[m - 1];
        while (++n <= n9) {
            const int r = n - m;
            Cell* h = H + r; Cell* f = F + r; Cell* f2 = F2 + r;
            const Cell* mx = h;
            const int diag = h->val, was_diag = is_diag(h->dir);
            h->val += sim(sc, x, p->b[n - 1]);
            h->dir = was_diag ? DIAG : NEWD;
            const Cell* from = h + 1;
            int v = from->val + sc->gop;
            if (v >= f[1].val) { f->val = v; f->ptr = from->ptr; f->dir = VERT; } else *f = f[1];
            f->val += sc->gep;
            if (f->val > mx->val) mx = f;
            if (dagp) {
                v = from->val + sc->lgop;
                if (v >= f2[1].val) { f2->val = v; f2->ptr = from->ptr; f2->dir = VERT; } else *f2 = f2[1];
                f2->val += sc->lgep;
                if (f2->val > mx->val) mx = f2;
            }
            v = h[-1].val + sc->gop;
            if (v >= e1.val) { e1.val = v; e1.ptr = h[-1].ptr; e1.dir = HORI; }
            e1.val += sc->gep;
            if (e1.val >= mx->val) mx = &e1;
            if (dagp) {
                v = h[-1].val + sc->lgop;
                if (v >= e2.val) { e2.val = v; e2.ptr = h[-1].ptr; e2.dir = HORL; }
                e2.val += sc->lgep;
                if (e2.val >= mx->val) mx = &e2;
            }
            if (mx != h) *h = *mx;
            else if (sc->local && h->val > diag) {
                if (LocalL && diag == 0) h->ptr = links_add(vmf, m - 1, n - 1, 0);
                else if (LocalR && h->val > best) { best = h->val; best_p = h->ptr; best_m = m; best_n = n; }
            }
            if (LocalL && h->val <= 0) h->val = h->dir = 0;
            else if (h->dir == NEWD) h->ptr = links_add(vmf, m - 1, n - 1, h->ptr);
        }
    }
    if (LocalR) *pp = links_add(vmf, best_m, best_n, best_p);
    else {
        /* lastB_ng */
        Cell* h9 = H + (br - ar);
        float f = p->b_exgr ? 0.f : up->tgapf;
        int dm = 0, dn = 0;
        if (br == p->b_len && f < 1) {
            int rw = w->up;
            if (br - al < rw) rw = br - al;
            for (Cell* h = H + rw; --h >= h9; ) {
                Cell* g = h + 1;
                ++dm;
                const int gpn = !is_vert(g->dir) ? gap_penalty(sc, 1) : gap_ext_pen(sc, dm);
                g->val += (int) (gpn * f);
                if (g->val > h->val) { *h = *g; h->dir = VERT; } else dm = 0;
            }
        }
        f = p->a_exgr ? 0.f : up->tgapf;
        if (ar == p->a_len && f < 1) {
            int rw = w->lw;
            if (bl - ar > rw) rw = bl - ar;
            for (Cell* h = H + rw; ++h <= h9; ) {
                Cell* g = h - 1;
                ++dn;
                const int gpn = !is_hori(g->dir) ? gap_penalty(sc, 1) : gap_ext_pen(sc, dn);
                g->val += (int) (gpn * f);
                if (g->val > h->val) { *h = *g; h->dir = VERT; } else dn = 0;
            }
        }
        if (dn || dm) {
            if (dn) dm = 0;
            h9->ptr = links_add(vmf, ar - dm, br - dn, h9->ptr);
        }
        h9->ptr = links_add(vmf, ar, br, h9->ptr);
        best = h9->val;
        *pp = h9->ptr;
    }
    free(buf);
    return best;
}

/* scorealoneB_ng */
int ubr_scorealone(const SpdpScoring* sc, const SpdpUnsplicedParams* up, const SpdpProblem* p)
{
    (void) up;
    SpdpWindow w;
    ubr_stripe(p, sc->sh, &w);
    const int dagp = sc->noll == 3;
    const int LocalL = sc->local && p->a_exgl && p->b_exgl, LocalR = sc->local && p->a_exgr && p->b_exgr;
    const int al = p->a_left, ar = p->a_right, bl = p->b_left, br = p->b_right;
    const int nol = dagp ? 3 : 2;
    if (w.width < 3) return NEVSEL;
    int* buf = (int*) malloc(sizeof(int) * (size_t) nol * w.width);
    for (int i = 0; i < nol * w.width; ++i) buf[i] = NEVSEL;
    int* H = buf - w.lw + 1;
    int* F = H + w.width;
    int* F2 = F + w.width;
    int best = NEVSEL;
    {   /* sinitB_ng */
        int r = bl - al, rr = br - al;
        H[r] = 0;
        if (p->a_exgl) {
            if (w.up < rr) rr = w.up;
            for (int q = r + 1; q <= rr; ++q) H[q] = 0;
        }
        rr = bl - ar;
        if (w.lw > rr) rr = w.lw;
        if (p->b_exgl) { for (int q = rr; q < r; ++q) H[q] = 0; }
        else for (int i = 1; --r >= rr; ++i) {
            H[r] = H[r + 1];
            if (i == 1) { H[r] += gap_penalty(sc, 1); F[r] = H[r]; }
            else { F[r] = F[r + 1]; H[r] += gap_ext_pen(sc, i); F[r] += sc->gep; }
        }
    }
    for (int m = p->a_exgl ? al + 1 : al; m <= ar; ++m) {
        int e1 = NEVSEL, e2 = NEVSEL;
        int n = m - 1 + w.lw;
        if (n < bl) n = bl;
        int n9 = m + w.up;
        if (n9 > br) n9 = br;
        const int x = m > al ? p->a[m - 1] : 0;
        while (++n <= n9) {
            const int r = n - m;
            int* h = H + r; int* f = F + r; int* f2 = F2 + r;
            const int* mx = h;
            int v;
            if (m != al) {
                *h += sim(sc, x, p->b[n - 1]);
                v = h[1] + sc->gop;
                *f = (v > f[1] ? v : f[1]) + sc->gep;
                if (*f > *mx) mx = f;
                if (dagp) {
                    v = h[1] + sc->lgop;
                    *f2 = (v > f2[1] ? v : f2[1]) + sc->lgep;
                    if (*f2 > *mx) mx = f2;
                }
            }
            v = h[-1] + sc->gop;
            e1 = (v > e1 ? v : e1) + sc->gep;
            if (e1 > *mx) mx = &e1;
            if (dagp) {
                v = h[-1] + sc->lgop;
                e2 = (v > e2 ? v : e2) + sc->lgep;
                if (e2 > *mx) mx = &e2;
            }
            const int y = *h;
            if (mx != h) *h = *mx;
            else if (LocalR && y > best) best = y;
            if (LocalL && *h < 0) *h = 0;
        }
    }
    if (!LocalR) {      /* slastB_ng */
        const int* h9 = H + (br - ar);
        best = *h9;
        if (p->b_exgr) {
            const int rw = w.up < br - al ? w.up : br - al;
            for (const int* h = H + rw; h > h9; --h) if (*h > best) best = *h;
        }
        if (p->a_exgr) {
            const int rw = w.lw > bl - ar ? w.lw : bl - ar;
            for (const int* h = H + rw; h < h9; ++h) if (*h > best) best = *h;
        }
    }
    free(buf);
    return best;
}

/* stdskl for single-residue rows: the records sorted by (m, n) are vertices of a monotone path; each step is a diagonal leg
 * followed by a gap leg; a vertex is a corner when the leg leaving it does not continue the leg arriving */
static int cmp_skl(const void* x, const void* y)
{
    const SpdpSkl* a = (const SpdpSkl*) x; const SpdpSkl* b = (const SpdpSkl*) y;
    return a->m != b->m ? (a->m < b->m ? -1 : 1) : (a->n < b->n ? -1 : (a->n > b->n));
}
static int corner_list(SpdpSkl* pts, int n, SpdpSkl* out)
{
    if (n < 2) { for (int i = 0; i < n; ++i) out[i] = pts[i]; return n; }
    qsort(pts, n, sizeof(SpdpSkl), cmp_skl);
    int k = 0, heading = 2, at = 0;
    for (int nx = 1; nx < n; ++nx) {
        const int am = pts[nx].m - pts[at].m, an = pts[nx].n - pts[at].n;
        if (an < 0 || (!am && !an)) continue;
        const int diag = am < an ? am : an, slack = an - am;
        const int gap = (slack > 0) - (slack < 0);
        const int two = diag && gap;
        if ((two ? 0 : gap) != heading || !am) out[k++] = pts[at];
        if (two) { out[k].m = pts[at].m + diag; out[k].n = pts[at].n + diag; ++k; }
        heading = gap;
        at = nx;
    }
    out[k++] = pts[at];
    return k;
}

int ubr_corner_list(SpdpSkl* pts, int n, SpdpSkl* out) { return corner_list(pts, n, out); }

/* globalB_ng with qck = 0: out[0] = header {m = 1, n = corners}, corners follow; returns the number of entries written
 * (0: no alignment); *score = what the reference leaves in gsi->scr */
int ubr_align(const SpdpScoring* sc, const SpdpUnsplicedParams* up, const SpdpProblem* p, SpdpSkl* out, int cap, int* score)
{
    SpdpWindow w;
    ubr_stripe(p, sc->sh, &w);
    const int m = p->a_right - p->a_left, n = p->b_right - p->b_left;
    Recs rec = {0, 0, 0};
    int scr = 0;
    if (!m && !n) scr = 0;
    else if (!m || !n) {
        recs_add(&rec, p->a_left, p->b_left);
        recs_add(&rec, p->a_right, p->b_right);
        if (m) scr = (p->b_exgl || p->a_exgr) ? gap_ext_pen(sc, m) : gap_penalty(sc, m);      /* (:1250 reads b's flag for "aexgl") */
        else scr = (p->b_exgl || p->b_exgr) ? gap_ext_pen(sc, n) : unp_penalty(sc, n);
    } else if (w.up == w.lw) {      /* diagonalB_ng */
        const int LocalL = sc->local && p->a_exgl && p->b_exgl, LocalR = sc->local && p->a_exgr && p->b_exgr;
        int best = NEVSEL, mL = p->a_left, mR = p->a_right, s = 0;
        const int d = p->b_left - p->a_left;
        for (int i = p->a_left; i < p->a_right; ) {
            s += sim(sc, p->a[i], p->b[i + d]);
            ++i;
            if (LocalL && s < 0) { s = 0; mL = i; }
            if (LocalR && s > best) { best = s; mR = i; }
        }
        recs_add(&rec, mL, mL + d);
        recs_add(&rec, mR, mR + d);
        scr = LocalR ? best : s;
    } else if (w.width < 0) scr = NEVSEL;
    else {                          /* trcbkalignB_ng */
        Links vmf = {0, 0, 0};
        int pp = 0;
        scr = forward(sc, up, p, &w, &vmf, &pp);
        if (pp) {
            int last_m = 0, last_n = 0;
            for (int q = pp; ; ) {
                recs_add(&rec, vmf.r[q].m, vmf.r[q].n);
                last_m = vmf.r[q].m; last_n = vmf.r[q].n;
                q = vmf.r[q].p;
                if (!q) break;
            }
            if (!sc->local && (last_m != p->a_left || last_n != p->b_left)) recs_add(&rec, p->a_left, p->b_left);
        }
        free(vmf.r);
    }
    *score = scr;
    int k = 0;
    if (rec.n && scr > NEVSEL && 2 * rec.n + 2 <= cap) {
        k = corner_list(rec.r, rec.n, out + 1);
        out[0].m = 1; out[0].n = k;
        ++k;
    }
    free(rec.r);
    return k;
}

/* skl_rngB_ng: skl = header + corners as ubr_align returns them (trimmed here as the reference does, on a copy);
 * edits (optional): cap records of {op, alen, blen} in the chosen format; sam[5] = flag, pos, mapq, left, right */
typedef struct { int32_t val, mch, mmc; float gap, unp; int32_t span; } UbrStat;
int ubr_rescore(const SpdpScoring* sc, const SpdpUnsplicedParams* up, const SpdpProblem* p, const SpdpSkl* skl, int n_skl,
                UbrStat* st, int format, SpdpEdit* ed, int cap, int* sam, SpdpSkl* trimmed, int* n_trimmed)
{
    memset(st, 0, sizeof *st);
    if (n_trimmed) *n_trimmed = 0;
    if (n_skl < 3) return 0;
    int num = n_skl - 1;
    SpdpSkl* c = (SpdpSkl*) malloc(sizeof(SpdpSkl) * (num + 1));
    memcpy(c, skl + 1, sizeof(SpdpSkl) * num);
    {   /* trimskl */
        int i = c[1].m - c[0].m, j = c[1].n - c[0].n;
        if ((p->a_exgl && !i) || (p->b_exgl && !j)) { memmove(c, c + 1, sizeof(SpdpSkl) * (num - 1)); --num; }
        if (num >= 2) {
            i = c[num - 1].m - c[num - 2].m; j = c[num - 1].n - c[num - 2].n;
            if ((p->a_exgr && !i) || (p->b_exgr && !j)) --num;
        }
    }
    if (trimmed) { memcpy(trimmed, c, sizeof(SpdpSkl) * num); *n_trimmed = num; }
    int ne = 0;
#define PUSH(o, x, y) do { if (ed && ne < cap) { ed[ne].op = (o); ed[ne].alen = (x); ed[ne].blen = (y); } ++ne; } while (0)
    int m = c[0].m, n = c[0].n, scr = 0, span = 0;
    if (format == SPDP_FMT_SAM) {
        if (sam) { sam[0] = 0; sam[1] = n; sam[3] = m; }
        if (m) PUSH('H', m, 0);
    }
    float tg = (m == 0 || n == 0) ? up->tgapf : 1.f;
    for (int q = 1; q < num; ++q) {
        const int mi = c[q].m - m, ni = c[q].n - n, i = mi - ni;
        int d = i >= 0 ? ni : mi;
        span += mi > ni ? mi : ni;
        if (d) {
            if (format == SPDP_FMT_VULGAR) PUSH('M', d, d); else if (format) PUSH('M', d, 0);
            for (int k = 0; k < d; ++k) {
                const int x = p->a[m + k], y = p->b[n + k];
                scr += sim(sc, x, y);
                if (x == y) ++st->mch; else ++st->mmc;
            }
            m += d; n += d;
        }
        if (i < 0) { d = -i; if (format == SPDP_FMT_VULGAR) PUSH('G', 0, d); else if (format) PUSH('D', d, 0); }
        else if (i > 0) { d = i; if (format == SPDP_FMT_VULGAR) PUSH('G', d, 0); else if (format) PUSH('I', d, 0); }
        else d = 0;
        if (d) {
            if (c[q].m == p->a_len || c[q].n == p->b_len) tg = up->tgapf;
            st->gap += tg;
            st->unp += d * tg;
            scr += (int) (gap_penalty(sc, d) * tg);
            tg = 1.f;
        }
        m = c[q].m; n = c[q].n;
    }
    if (format == SPDP_FMT_SAM) {
        if (m < p->a_len) PUSH('H', p->a_len - m, 0);
        if (sam) { sam[4] = m; sam[2] = 30 + (int) (100 * (st->mmc + st->unp) / p->a_len); }
    }
#undef PUSH
    st->val = scr;
    st->span = span;
    free(c);
    return ne;
}
