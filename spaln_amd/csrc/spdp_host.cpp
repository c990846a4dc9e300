// spdp_host.cpp -- the reference's dispatch around the DP engines, host side.
//
// What it mirrors (ogotoh/spaln v3.0.7):
//   alignS_ng (ori = 1, seeding off)        src/fwd2s1.cc:2746-2760
//   Aln2s1::globalS_ng                      src/fwd2s1.cc:2674-2694
//   Aln2s1::lspS_ng   (decision ladder)     src/fwd2s1.cc:1801-1897   (its decisions: spdp_ladder.h, shared with
//   Aln2s1::mimd_postwork / rcsv_postwork   src/fwd2s1.cc:1714-1799    the protein ladder of spdp_h_api.cpp)
//   Aln2s1::trcbkalignS_ng                  src/fwd2s1.cc:1667-1710
//   Aln2s1::diagonalS_ng                    src/fwd2s1.cc:1629-1665
//   stdskl / trimskl                        src/gaps.cc:140-180, 254-273
//
// The reference runs this ladder synchronously per query, deep inside its
// worker threads.  Here the same decisions are taken for a whole batch in
// rounds: every pending sub-problem is classified, all UDH sweeps of the round
// go to the GPU in one launch, their cpos rows are turned into slabs (or, in
// recursive mode, into two half problems for the next round), and finally all
// traceback sub-problems of all queries run in one forward launch + one walk.
// Sub-problems are descriptors into the resident inputs (no re-upload).

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <mutex>
#include <thread>

#include "spdp_internal.h"
#include "spdp_chunk_plan.h"
#include "spdp_ladder.h"

namespace {

const int kEndOfUlk = SPDP_END_OF_ULK;
const int kScalarRows = 8;                  // trcbkalignS_ng: m < 8 goes to the scalar engine

struct Rng { int al, ar, bl, br; uint8_t a_exgl, a_exgr, b_exgl, b_exgr; };

struct Job {                                // one query through alignS_ng
    int score = SPDP_NEVSEL;
    bool score_set = false;
    bool failed = false;
    bool edge = false;                      // a linear-space call of this query ran along the free left edge (SPDP_ALN_LEFT_EDGE)
    std::vector<SpdpSkl> rec;               // Mfile records after the dummy one
};

struct LspItem { int job; Rng r; SpdpWindow w; bool top; };
struct TbItem  { int job; Rng r; SpdpWindow w; bool top; int cut_l = 0, cut_r = 0; };     // trcbkalignS_ng call (cut_r > cut_l: with a cut range)
struct UdhItem { int job; Rng r; SpdpWindow w; bool top; int n_imd; bool recursive; int imd_intvl; };

Rng rng_of(const ladder::Slab& s) { return {s.al, s.ar, s.bl, s.br, 0, 0, (uint8_t) s.b_exgl, 0}; }

RunItem run_item(int parent, const Rng& r, const SpdpWindow& w, int n_im)
{
    RunItem it;
    it.parent = parent;
    it.a_left = r.al; it.a_right = r.ar; it.b_left = r.bl; it.b_right = r.br;
    it.a_exgl = r.a_exgl; it.a_exgr = r.a_exgr; it.b_exgl = r.b_exgl; it.b_exgr = r.b_exgr;
    it.w = w; it.n_im = n_im;
    return it;
}

// PwdB::GapPenalty / GapExtPen / UnpPenalty with codonk1 = LARGEN (Noll = 2), src/aln.h:275-287
int gap_penalty(const SpdpScoring& sc, int i) { return i == 0 ? 0 : sc.gop + i * sc.gep; }
int gap_ext_pen(const SpdpScoring& sc, int) { return sc.gep; }
int unp_penalty(const SpdpScoring& sc, int d) { return d * sc.gep; }

// Aln2s1::diagonalS_ng (non-local and local), src/fwd2s1.cc:1629-1665
int diagonal_s(const SpdpScoring& sc, const SpdpProblem& p, const Rng& r, std::vector<SpdpSkl>& rec)
{
    const bool Local = sc.local;
    const bool LocalL = Local && r.a_exgl && r.b_exgl;
    const bool LocalR = Local && r.a_exgr && r.b_exgr;
    const int dlt = Local ? 0 : ((r.br - r.bl) - (r.ar - r.al));
    // if dlt < 0 the roles of a and b are swapped for the walk
    const uint8_t* as = dlt < 0 ? p.b : p.a;
    const uint8_t* bs = dlt < 0 ? p.a : p.b;
    const int al = dlt < 0 ? r.bl : r.al, ar = dlt < 0 ? r.br : r.ar;
    const int bl = dlt < 0 ? r.al : r.bl;
    int mL = al, mR = ar;
    int scr = 0, maxh = SPDP_NEVSEL;
    for (int m = al; m++ < ar; ) {
        const int x = as[m - 1], y = bs[bl + (m - 1 - al)];
        scr += dlt < 0 ? sc.mtx[y * sc.mtx_dim + x] : sc.mtx[x * sc.mtx_dim + y];
        if (LocalL && scr < 0) { scr = 0; mL = m; }
        if (LocalR && scr > maxh) { maxh = scr; mR = m; }
    }
    int rr = bl - al;
    if (dlt < 0) rr -= dlt;
    // NB: the reference writes (m, n) of the *swapped* pair; reproduce literally
    rec.push_back({mL, mL + rr});
    rec.push_back({mR, mR + rr});
    return LocalR ? maxh : scr;
}

}   // namespace

// Corner list of a set of path records (what stdskl / stdskl3, src/gaps.cc:140-227, return; in / out without header).
// The records, sorted by (m, n), are the vertices of a monotone polyline.  Every step between two of them is a
// diagonal leg (when it advances in both sequences) followed by a gap leg (when the advances differ); a vertex is
// a corner when the leg leaving it does not continue the leg arriving -- plus, as in the reference, every vertex
// that starts a step without progress in m.  M_UNIT = 3 for protein rows against nucleotide columns: a gap leg that
// is not a whole number of codons rounds the row of its corner up (row gaps) or splits off the frame shift (column gaps).
template <int M_UNIT>
std::vector<SpdpSkl> corner_list(std::vector<SpdpSkl> pts)
{
    if (pts.size() < 2) return pts;
    std::sort(pts.begin(), pts.end(), [](const SpdpSkl& x, const SpdpSkl& y) { return x.m != y.m ? x.m < y.m : x.n < y.n; });
    std::vector<SpdpSkl> corners;
    corners.reserve(2 * pts.size() + 1);
    enum { DIAG = 0, NONE = 2 };                     // headings: 0 diagonal, +1 gap along n, -1 gap along m
    int heading = NONE;
    size_t at = 0;
    for (size_t nxt = 1; nxt < pts.size(); ++nxt) {
        const int adv_m = (pts[nxt].m - pts[at].m) * M_UNIT, adv_n = pts[nxt].n - pts[at].n;
        if (adv_n < 0 || (!adv_m && !adv_n)) continue;           // a step back or a repeat: not a vertex
        const int diag = std::min(adv_m, adv_n), slack = adv_n - adv_m;
        const int gap = (slack > 0) - (slack < 0);
        const bool two_legs = diag && gap;
        if ((two_legs ? (int) DIAG : gap) != heading || !adv_m) corners.push_back(pts[at]);
        if (two_legs) {
            SpdpSkl c;
            c.n = pts[at].n + diag;
            c.m = pts[at].m + (diag + ((M_UNIT > 1 && slack < 0 && slack % M_UNIT) ? M_UNIT - 1 : 0)) / M_UNIT;
            corners.push_back(c);
            if (M_UNIT > 1 && slack > 0 && slack % M_UNIT) { c.n += slack % M_UNIT; corners.push_back(c); }
        }
        heading = gap;
        at = nxt;
    }
    corners.push_back(pts[at]);
    return corners;
}
template std::vector<SpdpSkl> corner_list<1>(std::vector<SpdpSkl>);
template std::vector<SpdpSkl> corner_list<3>(std::vector<SpdpSkl>);

// host-only entry (no device work): the corner list of n records, out[] has room for 2 n + 1; returns the count
extern "C" int spdp_corner_list(const SpdpSkl* recs, int n, int m_unit, SpdpSkl* out)
{
    if (!recs || !out || n < 0 || (m_unit != 1 && m_unit != 3)) return -1;
    std::vector<SpdpSkl> v(recs, recs + n);
    v = m_unit == 1 ? corner_list<1>(std::move(v)) : corner_list<3>(std::move(v));
    std::copy(v.begin(), v.end(), out);
    return (int) v.size();
}

namespace {

// trimskl, src/gaps.cc:254-273: delete terminal gaps at free ends
void trim_skl(std::vector<SpdpSkl>& s, const SpdpProblem& p)
{
    if (s.size() >= 2) {
        const int i = s[1].m - s[0].m, j = s[1].n - s[0].n;
        if ((p.a_exgl && !i) || (p.b_exgl && !j)) s.erase(s.begin());
    }
    if (s.size() >= 2) {
        const size_t k = s.size() - 1;
        const int i = s[k].m - s[k - 1].m, j = s[k].n - s[k - 1].n;
        if ((p.a_exgr && !i) || (p.b_exgr && !j)) s.pop_back();
    }
}

}   // namespace
void trim_skl_of(std::vector<SpdpSkl>& s, const SpdpProblem& p) { trim_skl(s, p); }
namespace {

// Chunks of one batch run as a software pipeline on two lanes of the context (own streams and pools): chunk c starts
// its first linear-space sweep when that of chunk c - 1 has finished, so the host work, the slab tracebacks and the
// walk of one chunk run beside the big sweep of the next instead of leaving the GPU idle between launches.
// "Has finished" is stricter than needed: once every block of chunk c - 1's sweep has STARTED (SweepArgs::started), the
// next sweep can be launched with no dependency at all -- its blocks take the slots the last blocks of the sweep before
// it leave, where a wait for the event drains the GPU first.  The chunk's thread sees that signal in host memory and
// opens the gate with GATE_LAUNCH_NOW; a launch that cannot carry the signal, or whose signal was not seen before
// the sweep ended, opens it with GATE_EVENT as before.
enum GateState : int { GATE_SHUT = 0, GATE_EVENT = 1, GATE_NONE = 2, GATE_LAUNCH_NOW = 3 };
struct ChunkGate {
    std::mutex m;
    std::condition_variable cv;
    int state = GATE_SHUT;                      // GATE_EVENT: wait for `ev` on the device; GATE_NONE: nothing to wait for
    int opened = 0;                             // open() calls, the closing GATE_NONE of Aligner::run on an open gate apart
    hipEvent_t ev = nullptr;
    void open(int st_)
    {
        {
            std::lock_guard<std::mutex> g(m);
            if (state == GATE_SHUT || st_ != GATE_NONE) ++opened;
            if (state == GATE_SHUT) state = st_;
        }
        cv.notify_all();
    }
    int wait() { std::unique_lock<std::mutex> g(m); cv.wait(g, [&] { return state != GATE_SHUT; }); return state; }
};

// the default plan of a big batch (align_on_store): chosen from the grid in profiles/chunk_lanes_c2.txt.  With the lanes'
// copies waiting for their own stream only, what follows the last sweep is the last chunk's post-work alone, so that chunk
// is the smaller one; a third chunk still loses (a lane's next sweep waits for the post-work of its chunk before)
constexpr int    kDefaultChunks = 2;
constexpr double kDefaultChunkRatio = 0.55;

struct Aligner {
    SpdpContext* ctx;                           // the lane this chunk runs on
    const DevStore* st;
    const SpdpProblem* probs;                   // first problem of the chunk
    int n;
    int base = 0;                               // its index in the store (parent of job j = base + j)
    ChunkGate* gate_in = nullptr;               // the chunk before mine / mine
    ChunkGate* gate_out = nullptr;
    SpdpAlignment* out = nullptr;               // where the chunk's alignments go (may be null)
    bool raw = false;                           // lspS_ng level: hand the Mfile records over as they are
    const SpdpRequests* req = nullptr;          // explicit engine calls on sub-ranges of store entries (the seeded path)
    int parent(int job) const { return req ? req->parents[base + job] : base + job; }
    std::vector<TbItem> ctbs;                   // forwardS_ng calls with a cut range
    std::vector<Job> jobs;
    std::vector<LspItem> pending;
    std::vector<TbItem> tbs;                    // forwardS1_wip calls
    std::vector<TbItem> stbs;                   // scalar forwardS_ng calls (< 8 rows)
    std::vector<TbItem> xtbs;                   // -A1: forwardS1 calls
    float kernel_ms = 0.f;
    int64_t kernel_cells = 0;
    int unsupported = 0;
    int overflowed = 0;                         // queries given up because a record list did not fit (scalar / -A1 walkers)
    double stats[SPDP_N_STATS] = {0};           // see include/spdp.h

    void set_score(int job, bool top, int scr) { if (top) { jobs[job].score = scr; jobs[job].score_set = true; } }

    // Aln2s1::trcbkalignS_ng
    // a sub-range the links produced that does not lie inside the sequences: the reference would run
    // its engine on it anyway (out-of-bounds reads); here the query is reported as not aligned
    bool bad_range(int job, const Rng& r) const
    {
        return r.al < 0 || r.bl < 0 || r.ar > probs[job].a_len || r.br > probs[job].b_len || r.ar < r.al || r.br < r.bl;
    }

    void trcbk(int job, const Rng& r, const SpdpWindow& w, bool top)
    {
        if (w.width < 0) { set_score(job, top, SPDP_NEVSEL); return; }
        if (bad_range(job, r) || w.width < 3) { ++unsupported; jobs[job].failed = true; return; }
        if (st->sc.scalar_engines == 1 || r.ar - r.al < kScalarRows) {   // -A0, or fewer than 8 rows: scalar forwardS_ng (src/fwd2s1.cc:1677)
            if (!st->has_exact) { ++unsupported; jobs[job].failed = true; return; }
            stbs.push_back({job, r, w, top});
            return;
        }
        if (st->sc.scalar_engines == 2) {       // -A1: forwardS1 (mode 3 / 5) + Vmf::traceback
            if (!st->has_exact) { ++unsupported; jobs[job].failed = true; return; }
            xtbs.push_back({job, r, w, top});
            return;
        }
        tbs.push_back({job, r, w, top});
    }

    // Aln2s1::lspS_ng up to the point where an engine is needed
    void classify(const LspItem& it, std::vector<UdhItem>& udh)
    {
        const SpdpScoring& sc = st->sc;
        const Rng& r = it.r;
        Job& J = jobs[it.job];
        const ladder::Plan pl = ladder::plan<1>(r.al, r.ar, r.bl, r.br, it.w,
                                                {sc.scalar_engines, sc.recursive, sc.ubh, sc.max_vmf_space, sc.noll});
        switch (pl.kind) {
        case ladder::EMPTY: set_score(it.job, it.top, 0); return;
        case ladder::ONE_SEQUENCE: {
            const int m = r.ar - r.al, n = r.br - r.bl;
            J.rec.push_back({r.al, r.bl});
            J.rec.push_back({r.ar, r.br});
            int scr;
            if (m) scr = (r.a_exgl || r.a_exgr) ? gap_ext_pen(sc, m) : gap_penalty(sc, m);
            else   scr = (r.b_exgl || r.b_exgr) ? gap_ext_pen(sc, n) : unp_penalty(sc, n);
            set_score(it.job, it.top, scr);
            return;
        }
        case ladder::DIAGONAL: set_score(it.job, it.top, diagonal_s(sc, probs[it.job], r, J.rec)); return;
        case ladder::TRACEBACK: trcbk(it.job, r, it.w, it.top); return;
        }
        if (bad_range(it.job, r) || it.w.width < 3) { ++unsupported; J.failed = true; return; }
        if ((sc.scalar_engines == 1 || sc.scalar_engines == 2) && !st->has_exact) { ++unsupported; J.failed = true; return; }
        udh.push_back({it.job, r, it.w, it.top, pl.n_imd, pl.recursive != 0, pl.imd_intvl});
    }

    double t_mark = 0;
    bool timing = getenv("SPDP_TIMING") != nullptr;
    void lap(const char* what)
    {
        if (!timing) return;
        const double now = std::chrono::duration<double, std::milli>(
            std::chrono::steady_clock::now().time_since_epoch()).count();
        if (t_mark > 0) fprintf(stderr, "[spdp timing] %-28s %8.2f ms\n", what, now - t_mark);
        t_mark = now;
    }

    // the launch's "all blocks started" word, looked at until it is set or the sweep has ended (its end event bounds the
    // wait: a word that never comes costs nothing but the old behaviour)
    static bool started(const DevRun& run)
    {
        if (!run.signal_armed) return false;
        const int* word = run.ctx->sig_host;
        for (unsigned look = 0; !__atomic_load_n(word, __ATOMIC_ACQUIRE); ++look) {
            if (look % 16 == 15 && hipEventQuery(run.eve()) != hipErrorNotReady) return __atomic_load_n(word, __ATOMIC_ACQUIRE) != 0;
            std::this_thread::sleep_for(std::chrono::microseconds(30));
        }
        return true;
    }

    int run()
    {
        const int rc = run_chunk();
        if (gate_out) gate_out->open(GATE_NONE);        // no linear-space round (or an error): the next chunk need not wait
        if (!rc && out) for (int i = 0; i < n; ++i) finish(i, out + i);     // stdskl / trimskl, beside the other chunks
        return rc;
    }

    int run_chunk()
    {
        const SpdpScoring& sc = st->sc;
        lap("start");
        jobs.assign(n, Job());
        for (int i = 0; i < n; ++i) {           // alignS_ng: stripe(alprm.sh), globalS_ng -> lspS_ng
            const SpdpProblem& p = probs[i];
            Rng r{p.a_left, p.a_right, p.b_left, p.b_right, p.a_exgl, p.a_exgr, p.b_exgl, p.b_exgr};
            SpdpWindow w;
            ladder::stripe<1>(r.al, r.ar, r.bl, r.br, sc.sh, &w);
            if (req) {                          // a caller that made the reference's decisions up to the engine call itself
                w = req->windows[base + i];
                const int kind = req->kinds[base + i];
                if (kind == 1) { trcbk(i, r, w, true); continue; }
                if (kind == 2) {                // trcbkalignS_ng(wdw, spj, mc): always the scalar engine (src/fwd2s1.cc:1674-1678)
                    if (w.width < 0) { set_score(i, true, SPDP_NEVSEL); continue; }
                    if (bad_range(i, r) || !st->has_exact) { ++unsupported; jobs[i].failed = true; continue; }
                    TbItem t{i, r, w, true};
                    t.cut_l = req->cuts[2 * (base + i)]; t.cut_r = req->cuts[2 * (base + i) + 1];
                    ctbs.push_back(t);
                    continue;
                }
            }
            pending.push_back({i, r, w, true});
        }
        // Queries that go straight to the traceback do not wait for the linear-space rounds of the others: their
        // forward sweep starts on the side stream as soon as the first classification is done (an EST batch
        // has a handful of stragglers in the linear-space engine; that launch is latency-bound and would
        // otherwise hold up everything).  SPDP_OVERLAP=0 restores the single-stream order.
        DevRun side(ctx);
        std::vector<TbItem> side_tbs;
        bool may_overlap = ctx->stream2 != nullptr && spdp_knob_on("SPDP_OVERLAP");
        bool first_round = true;
        while (!pending.empty()) {
            std::vector<LspItem> cur;
            cur.swap(pending);
            std::vector<UdhItem> udh;
            for (const LspItem& it : cur) classify(it, udh);
            lap("classify");
            if (may_overlap && !udh.empty() && tbs.size() >= 64) {
                side_tbs.swap(tbs);
                std::vector<RunItem> items;
                for (const TbItem& t : side_tbs) { items.push_back(run_item(parent(t.job), t.r, t.w, 0)); items.back().vmf_scale = 1 << 20; }   // (a few rows each)
                side.side = true;
                if (side.build(st, items, RUN_WIP_FORWARD) || side.launch()) return -1;
                lap("side fwd build+launch");
            }
            may_overlap = false;                        // first round only
            if (udh.empty()) continue;
            std::vector<RunItem> items;
            for (const UdhItem& u : udh) {
                items.push_back(run_item(parent(u.job), u.r, u.w, u.n_imd));
                items.back().imd_intvl = u.imd_intvl;
            }
            DevRun run(ctx);
            run.beside = !side_tbs.empty();
            const bool a0 = sc.scalar_engines == 1;
            if (run.build(st, items, a0 ? RUN_A0_UDH : (sc.scalar_engines == 2 ? RUN_A1_UDH : RUN_WIP_UDH))) return -1;
            lap("udh build");
            if (first_round && gate_in && gate_in->wait() == GATE_EVENT) HIPCHK(hipStreamWaitEvent(run.strm(), gate_in->ev, 0));
            run.signal_start = first_round && gate_out;
            if (run.launch()) return -1;
            if (first_round && gate_out) {
                HIPCHK(hipEventRecord(gate_out->ev, run.strm()));
                gate_out->open(started(run) ? GATE_LAUNCH_NOW : GATE_EVENT);
            }
            first_round = false;
            if (run.sync()) return -1;
            lap("udh launch+sync");
            kernel_ms += run.kernel_ms; kernel_cells += run.total_cells;
            stats[0] += run.kernel_ms; stats[1] += (double) run.total_cells; stats[2] += (double) items.size();
            stats[6] += 1;
            std::vector<int32_t> scores, cpos, ranges;
            std::vector<int32_t> edge;
            if (run.fetch_udh(scores, cpos, ranges, &edge)) return -1;
            std::vector<DevResult> ures;
            if (a0 && run.fetch_results(ures)) return -1;
            lap("udh fetch");
            const int stride = run.cpos_stride();
            for (size_t k = 0; k < udh.size(); ++k) {
                const UdhItem& u = udh[k];
                const int scr = scores[k];
                if (a0 && ures[k].pad[0]) { ++unsupported; jobs[u.job].failed = true; continue; }   // undefined in the reference
                set_score(u.job, u.top, scr);
                if (edge[k]) jobs[u.job].edge = true;
                if (scr <= SPDP_NEVSEL) continue;
                const int32_t* rg = &ranges[4 * k];          // ranges as written back by the engine
                const int32_t* cp = cpos.data() + k * stride;
                std::vector<SpdpSkl>& rec = jobs[u.job].rec;
                auto sink = ladder::sink([&](int m, int n) { rec.push_back({m, n}); },
                                         [&](const ladder::Slab& s) { trcbk(u.job, rng_of(s), s.w, false); return true; },
                                         [&](const ladder::Slab& s) { pending.push_back({u.job, rng_of(s), s.w, false}); });
                if (cp[0] == kEndOfUlk) {                       // does not cross an intermediate row
                    rec.push_back({rg[0], rg[2]});
                    rec.push_back({rg[1], rg[3]});
                } else ladder::postwork<1>(u.recursive, a0, sc.local, sc.sh, {rg[0], rg[1], rg[2], rg[3]}, 0, 0, u.n_imd, cp, sink);
            }
        }
        lap("postwork (slab lists)");
        // forwardS_ng (-A0, and any sub-problem below 8 rows) and forwardS1 (-A1) keep their traceback as Vmf records,
        // up to two per cell: a whole batch of slabs can ask for more memory than the card has, so they run in
        // groups whose record space stays below SPDP_VMF_GB (default 32) gigabytes
        auto run_vmf = [&](std::vector<TbItem>& list, RunFlavour flav, const char* what) -> int {
            size_t limit = (size_t) 32 << 30;
            if (const char* e = getenv("SPDP_VMF_GB")) limit = (size_t) std::max(1, atoi(e)) << 30;
            auto bytes_of = [](const TbItem& t, int scale) {
                return (size_t) vmf_capacity(t.r.ar - t.r.al + 1, t.r.br - t.r.bl + 1, t.w.width, scale) * sizeof(int3);
            };
            std::vector<size_t> todo(list.size());
            for (size_t k = 0; k < list.size(); ++k) todo[k] = k;
            for (int scale = 1; !todo.empty(); scale *= 8) {
                std::vector<size_t> again;
                for (size_t lo = 0; lo < todo.size(); ) {
                    size_t hi = lo, sum = 0;
                    while (hi < todo.size() && (hi == lo || sum + bytes_of(list[todo[hi]], scale) <= limit))
                        sum += bytes_of(list[todo[hi++]], scale);
                    std::vector<RunItem> items;
                    for (size_t k = lo; k < hi; ++k) {
                        const TbItem& t = list[todo[k]];
                        items.push_back(run_item(parent(t.job), t.r, t.w, 0));
                        items.back().vmf_scale = scale;
                        items.back().cut_l = t.cut_l; items.back().cut_r = t.cut_r;
                    }
                    DevRun run(ctx);
                    if (run.build(st, items, flav) || run.launch() || run.sync()) return -1;
                    kernel_ms += run.kernel_ms; kernel_cells += run.total_cells;
                    stats[3] += run.kernel_ms; stats[4] += (double) run.total_cells; stats[5] += (double) items.size();
                    std::vector<DevResult> res;
                    std::vector<int> nskl;
                    std::vector<int64_t> off;
                    std::vector<SpdpSkl> skl;
                    if (run.fetch_results(res) || run.fetch_skl(nskl, off, skl)) return -1;
                    for (size_t k = lo; k < hi; ++k) {
                        const TbItem& t = list[todo[k]];
                        const int c = nskl[k - lo];
                        if (c == -3 && scale < 4096) { again.push_back(todo[k]); continue; }     // outgrew its record budget: once more, larger
                        if (c == -1) { jobs[t.job].failed = true; ++overflowed; continue; }    // record list beyond its slot: this query only
                        if (c < 0) { ctx->err = what; return -1; }
                        set_score(t.job, t.top, res[k - lo].score);
                        const SpdpSkl* sk = skl.data() + off[k - lo];
                        jobs[t.job].rec.insert(jobs[t.job].rec.end(), sk, sk + c);
                    }
                    lo = hi;
                }
                todo.swap(again);
            }
            return 0;
        };
        if (!stbs.empty() && run_vmf(stbs, RUN_A0_FORWARD, "forwardS_ng traceback failed")) return -1;
        if (!ctbs.empty() && run_vmf(ctbs, RUN_A0_FORWARD, "forwardS_ng (cut range) traceback failed")) return -1;
        if (!xtbs.empty() && run_vmf(xtbs, RUN_A1_FORWARD, "forwardS1 traceback failed")) return -1;
        // all (remaining) trcbkalignS_ng calls of all queries: one forward sweep + one walk (beside the side run, if any)
        // A few tall slabs among many short ones (the recursion on a long cDNA leaves slabs of thousands of rows whose band
        // is narrow enough for the traceback): the launch would end with its tallest problem on the four waves of one
        // block.  They go to the side stream as a launch of their own -- all of them tall, so each gets a 16-wave block
        // (DevRun::build) -- beside the launch of the rest.  SPDP_SPLIT_FWD=0: one launch.
        if (side_tbs.empty() && ctx->stream2 != nullptr && tbs.size() > 1 && spdp_knob_on("SPDP_SPLIT_FWD")) {
            const int tall = 4 * 32 * SPDP_NELEM;               // >= 32 passes: DevRun::build's condition for 16-wave blocks
            std::vector<TbItem> rest;
            for (const TbItem& t : tbs) (t.r.ar - t.r.al >= tall ? side_tbs : rest).push_back(t);
            if (side_tbs.empty() || rest.empty() || (int) side_tbs.size() > 2 * ctx->n_cu) side_tbs.clear();
            else {
                tbs.swap(rest);
                std::vector<RunItem> items;
                for (const TbItem& t : side_tbs) items.push_back(run_item(parent(t.job), t.r, t.w, 0));
                side.side = true;
                if (side.build(st, items, RUN_WIP_FORWARD) || side.launch()) return -1;
                lap("tall fwd build+launch");
            }
        }
        // the scores and records of a finished `_wip` forward run into the jobs of its items
        auto collect = [&](DevRun& r, const std::vector<TbItem>& list, const char* fetched) -> int {
            kernel_ms += r.kernel_ms; kernel_cells += r.total_cells;
            stats[3] += r.kernel_ms; stats[4] += (double) r.total_cells; stats[5] += (double) list.size();
            stats[7] += (double) r.tb_bytes;
            std::vector<DevResult> res;
            std::vector<int> nskl;
            std::vector<int64_t> off;
            std::vector<SpdpSkl> skl;
            if (r.fetch_results(res) || r.fetch_skl(nskl, off, skl)) return -1;
            if (fetched) lap(fetched);
            for (size_t k = 0; k < list.size(); ++k) {
                const TbItem& t = list[k];
                if (nskl[k] == -1) { jobs[t.job].failed = true; ++overflowed; continue; }    // record list beyond its slot: this query only
                if (nskl[k] < 0) { ctx->err = "traceback walk failed"; return -1; }
                set_score(t.job, t.top, res[k].score);
                const SpdpSkl* s = skl.data() + off[k];
                jobs[t.job].rec.insert(jobs[t.job].rec.end(), s, s + nskl[k]);
            }
            return 0;
        };
        if (!tbs.empty()) {
            std::vector<RunItem> items;
            for (const TbItem& t : tbs) items.push_back(run_item(parent(t.job), t.r, t.w, 0));
            DevRun run(ctx);
            run.beside = !side_tbs.empty();
            if (run.build(st, items, RUN_WIP_FORWARD)) return -1;
            lap("fwd build");
            if (run.launch() || run.sync()) return -1;
            lap("fwd launch+sync (+walk)");
            if (collect(run, tbs, "fwd fetch")) return -1;
        }
        if (!side_tbs.empty()) {                        // collect the side run (its own pool: the runs above went on beside it)
            if (side.sync()) return -1;
            lap("side fwd sync");
            if (collect(side, side_tbs, nullptr)) return -1;
        }
        lap("assemble records");
        return 0;
    }

    // globalS_ng tail: header, stdskl, trimskl
    void finish(int i, SpdpAlignment* out) const
    {
        const Job& J = jobs[i];
        out->score = J.score_set ? J.score : SPDP_NEVSEL;
        out->n_skl = 0; out->skl = nullptr;
        out->flags = J.edge ? SPDP_ALN_LEFT_EDGE : 0;
        if (raw) {                              // what lspS_ng appended to the caller's Mfile (no header, any order)
            if (J.failed && req) { out->n_skl = -1; return; }   // (explicit requests: the caller must tell "no records" from "not served")
            if (J.failed || J.rec.empty()) return;
            out->n_skl = (int) J.rec.size();
            out->skl = (SpdpSkl*) malloc(sizeof(SpdpSkl) * J.rec.size());
            memcpy(out->skl, J.rec.data(), sizeof(SpdpSkl) * J.rec.size());
            return;
        }
        if (J.failed || (int) J.rec.size() < 2) return;
        std::vector<SpdpSkl> s = corner_list<1>(J.rec);
        trim_skl(s, probs[i]);
        out->n_skl = (int) s.size() + 1;
        out->skl = (SpdpSkl*) malloc(sizeof(SpdpSkl) * out->n_skl);
        out->skl[0].m = 1;                      // AlgnTrb
        out->skl[0].n = (int) s.size();
        memcpy(out->skl + 1, s.data(), sizeof(SpdpSkl) * s.size());
    }
};

}   // namespace

// ---- resident batches -----------------------------------------------------------------------
struct SpdpBatch {
    SpdpContext* ctx = nullptr;
    DevStore store;
    std::vector<SpdpProblem> probs;
    DevRun score;                                // HomScoreS_ng leg, built once
    bool score_built = false;
    double stats[SPDP_N_STATS] = {0};
};

int spdp_chunk_plan(const int64_t* cells, int n, int max_chunks, double ratio, int min_chunk, int* bounds)
{
    if (!cells || !bounds) return 0;
    return spdp_chunk_plan_of(cells, n, std::max(1, max_chunks), ratio, min_chunk, bounds);
}

SpdpBatch* spdp_batch_upload(SpdpContext* ctx, const SpdpScoring* sc, const SpdpProblem* probs, int n)
{
    if (!ctx || n <= 0) return nullptr;
    SpdpBatch* b = new SpdpBatch();
    b->ctx = ctx;
    b->probs.assign(probs, probs + n);
    if (b->store.upload(ctx, sc, probs, n)) { delete b; return nullptr; }
    return b;
}

void spdp_batch_free(SpdpBatch* bt) { delete bt; }

int64_t spdp_batch_cells(const SpdpBatch* bt)
{
    if (!bt) return 0;
    int64_t c = 0;
    for (const SpdpProblem& p : bt->probs) {
        SpdpWindow w;
        spdp_stripe(&p, bt->store.sc.sh, &w);
        c += spdp_cells(&p, &w);
    }
    return c;
}

int spdp_batch_homscore(SpdpBatch* bt, int32_t* scores, float* kernel_ms)
{
    if (!bt) return -1;
    {   // descriptors are rebuilt per call: work buffers live in the context's pool
        std::vector<RunItem> items;
        for (size_t i = 0; i < bt->probs.size(); ++i)
            items.push_back(spdp_item_of(bt->probs[i], (int) i, bt->store.sc.sh));
        if (bt->score.build(&bt->store, items, RUN_WIP_SCORE)) return -1;
    }
    if (bt->score.launch() || bt->score.sync()) return -1;
    if (kernel_ms) *kernel_ms = bt->score.kernel_ms;
    if (scores) {
        std::vector<DevResult> r;
        if (bt->score.fetch_results(r)) return -1;
        for (size_t i = 0; i < r.size(); ++i) scores[i] = r[i].score;
    }
    return 0;
}

static int align_on_store(SpdpContext* ctx, const DevStore* st, const SpdpProblem* probs, int n,
                          SpdpAlignment* out, float* kernel_ms, int64_t* kernel_cells,
                          double* stats = nullptr, bool raw = false, const SpdpRequests* req = nullptr)
{
    // big batches run as chunks on two lanes of the context, a software pipeline (ChunkGate); SPDP_CHUNKS=<n>: at most n
    // chunks, 1 turns it off; SPDP_CHUNK_RATIO=<r>: chunk c + 1 holds r times the DP cells of chunk c (spdp_chunk_plan.h).
    // Without SPDP_CHUNKS a chunk holds at least one residency round of problems (five 4-wave blocks per CU).
    int max_chunks = n >= 4096 ? kDefaultChunks : 1, min_chunk = 5 * std::max(1, ctx->n_cu);
    double ratio = kDefaultChunkRatio;
    if (const char* e = getenv("SPDP_CHUNKS")) { max_chunks = std::max(1, std::min(atoi(e), 8)); min_chunk = SPDP_CHUNK_LEAST; }
    if (const char* e = getenv("SPDP_CHUNK_RATIO")) ratio = atof(e);
    // a request batch runs on the dispatcher lane that took it, as ONE chunk: chunk lanes are spdp_lane(ctx, c), and for
    // the seeded dispatchers those are the contexts their sibling dispatchers run on from their own threads
    if (req) max_chunks = 1;
    std::vector<int> bounds((size_t) max_chunks + 1, 0);
    int n_chunks = 1;
    bounds[1] = n;
    if (max_chunks > 1 && n >= 2 * SPDP_CHUNK_LEAST) {
        std::vector<int64_t> cells(n);
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < n; ++i) {
            SpdpWindow w;
            spdp_stripe(&probs[i], st->sc.sh, &w);
            cells[i] = spdp_cells(&probs[i], &w);
        }
        n_chunks = spdp_chunk_plan_of(cells.data(), n, max_chunks, ratio, min_chunk, bounds.data());
        if (const char* e = getenv("SPDP_CHUNK_TEST_LAST"))     // test hook: the last chunk keeps its last <k> problems only
            if (n_chunks > 1) bounds[n_chunks - 1] = std::max(bounds[n_chunks - 1], n - std::max(1, atoi(e)));
        if (getenv("SPDP_TIMING"))
            fprintf(stderr, "[spdp timing] %-28s %8.2f ms  (%d chunks)\n", "chunk plan (cells + bounds)",
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), n_chunks);
    }
    const int n_lanes = std::min(n_chunks, 2);  // lane L runs chunks L, L + 2, .. one after the other; the gates chain c -> c + 1
    // a plan of shrinking chunks (ratio < 1) comes with blocking copies that wait for the lane's own stream only
    // (spdp_internal.h, at spdp_copy_sync): a chunk's post-work runs beside the next chunk's sweep, and only the last,
    // smaller chunk's is left behind the last sweep.  Equal chunks keep the null-stream copies: the same post-work under
    // a sweep measured 2.5 ms slower there (MEASUREMENTS).  SPDP_CHUNK_LANE_COPIES=1 / =0 sets the copies for any plan
    const char* lane_env = getenv("SPDP_CHUNK_LANE_COPIES");
    const bool own_copies = t_lane_copies || (n_chunks > 1 && (lane_env ? atoi(lane_env) != 0 : ratio > 0. && ratio < 1.));
    std::vector<Aligner> al(n_chunks);
    std::vector<ChunkGate> gates(n_chunks);
    std::vector<int> rc(n_chunks, 0);
    for (int c = 0; c < n_chunks; ++c) {
        Aligner& a = al[c];
        a.ctx = spdp_lane(ctx, c % 2);
        if (!a.ctx) { ctx->err = "cannot create a lane context"; return -1; }
        a.st = st;
        a.base = bounds[c];
        a.n = bounds[c + 1] - bounds[c];
        a.probs = probs + a.base;
        a.out = out ? out + a.base : nullptr;
        a.raw = raw;
        a.req = req;
        if (c + 1 < n_chunks) {                 // (the last chunk has nobody to open a gate for)
            if (hipEventCreateWithFlags(&gates[c].ev, hipEventDisableTiming) != hipSuccess) {
                for (int k = 0; k < c; ++k) if (gates[k].ev) (void) hipEventDestroy(gates[k].ev);
                ctx->err = "hipEventCreate"; return -1;
            }
            a.gate_out = &gates[c];
        }
        a.gate_in = c > 0 ? &gates[c - 1] : nullptr;
    }
    // a lane's chunks in turn; after a failure the gates of its remaining chunks are opened, so that no other lane waits
    auto run_lane = [&](int lane) {
        bool failed = false;
        for (int c = lane; c < n_chunks; c += n_lanes) {
            if (!failed) failed = (rc[c] = al[c].run()) != 0;
            else { rc[c] = -1; if (al[c].gate_out) al[c].gate_out->open(GATE_NONE); }     // (the lane's err is the failed chunk's)
        }
    };
    std::vector<std::thread> workers;
    for (int l = 1; l < n_lanes; ++l)
        workers.emplace_back([&, l]() { (void) hipSetDevice(ctx->device); LaneCopies own_stream(own_copies); run_lane(l); });
    { LaneCopies own_stream(own_copies); run_lane(0); }
    for (std::thread& t : workers) t.join();
    ctx->chunk_stats[0] += 1; ctx->chunk_stats[1] += n_chunks;
    for (int c = 0; c + 1 < n_chunks; ++c) {
        const int how = gates[c].state;
        ctx->chunk_stats[how == GATE_LAUNCH_NOW ? 2 : how == GATE_EVENT ? 3 : 4] += 1;
        if (gates[c].opened == 1) ctx->chunk_stats[5] += 1;
    }
    for (int c = 0; c < n_chunks; ++c) if (gates[c].ev) (void) hipEventDestroy(gates[c].ev);
    int unsupported = 0, overflowed = 0;
    float kms = 0.f; int64_t kc = 0;
    double st_sum[SPDP_N_STATS] = {0};
    for (int c = 0; c < n_chunks; ++c) {
        if (rc[c]) {                            // alignments other chunks have already handed over do not outlive the failed call
            if (al[c].ctx != ctx) ctx->err = al[c].ctx->err;
            if (out) spdp_free_alignments(out, n);
            return -1;
        }
        kms += al[c].kernel_ms; kc += al[c].kernel_cells; unsupported += al[c].unsupported; overflowed += al[c].overflowed;
        for (int k = 0; k < SPDP_N_STATS; ++k) st_sum[k] += al[c].stats[k];
    }
    if (kernel_ms) *kernel_ms = kms;
    if (kernel_cells) *kernel_cells = kc;
    if (stats) memcpy(stats, st_sum, sizeof st_sum);
    if (unsupported) {
        ctx->err = "sub-problems with fewer than 8 query rows need the scalar exact engine: supply "
                   "SpdpScoring.intpen / t53 and SpdpProblem.cano5 / cano3 / dinc";
        return 1;                               // partial: those queries are returned without alignment
    }
    if (overflowed) {
        ctx->err = "traceback record list of a scalar / -A1 engine call exceeds its slot; those queries come back without an alignment";
        return 1;
    }
    return 0;
}

int spdp_batch_align(SpdpBatch* bt, SpdpAlignment* out, float* kernel_ms, int64_t* kernel_cells)
{
    if (!bt) return -1;
    return align_on_store(bt->ctx, &bt->store, bt->probs.data(), (int) bt->probs.size(), out,
                          kernel_ms, kernel_cells, bt->stats);
}

int spdp_batch_stats(const SpdpBatch* bt, double* out, int n)
{
    if (!bt || !out) return -1;
    for (int i = 0; i < n && i < SPDP_N_STATS; ++i) out[i] = bt->stats[i];
    return 0;
}

int spdp_align_s(SpdpContext* ctx, const SpdpScoring* sc, const SpdpProblem* probs, int n_probs,
                 SpdpAlignment* out)
{
    if (!ctx) return -1;
    for (int i = 0; i < n_probs; ++i) { out[i].score = SPDP_NEVSEL; out[i].n_skl = 0; out[i].skl = nullptr; out[i].flags = 0; out[i].reserved = 0; }
    if (n_probs <= 0) return 0;
    DevStore st;
    if (st.upload(ctx, sc, probs, n_probs)) return -1;
    return align_on_store(ctx, &st, probs, n_probs, out, nullptr, nullptr);
}

// Aln2s1::lspS_ng (src/fwd2s1.cc:1817-1880) for a caller that keeps the record file itself (seededS_ng / interpolateS):
// the whole ladder below it, records as written (out[i].skl has no header record; globalS_ng's stdskl sorts them)
int spdp_lsp_s(SpdpContext* ctx, const SpdpScoring* sc, const SpdpProblem* probs, int n_probs, SpdpAlignment* out)
{
    if (!ctx || !sc || !out) return -1;
    for (int i = 0; i < n_probs; ++i) { out[i].score = SPDP_NEVSEL; out[i].n_skl = 0; out[i].skl = nullptr; out[i].flags = 0; out[i].reserved = 0; }
    if (n_probs <= 0) return 0;
    DevStore st;
    if (st.upload(ctx, sc, probs, n_probs)) return -1;
    return align_on_store(ctx, &st, probs, n_probs, out, nullptr, nullptr, nullptr, true);
}

// engine calls a caller has already dispatched itself (the seeded walk, spdp_seeded.cpp): request k runs lspS_ng (kind 0)
// or trcbkalignS_ng (kind 1; kind 2 with a cut range) on probs[k]'s ranges with windows[k], on the resident inputs of
// store entry parents[k]; out[k]: score + records as written, n_skl = -1 where the request could not be served
int spdp_run_requests(SpdpContext* ctx, const DevStore* st, const SpdpProblem* probs, int n, const SpdpRequests* req,
                      SpdpAlignment* out)
{
    for (int i = 0; i < n; ++i) { out[i].score = SPDP_NEVSEL; out[i].n_skl = 0; out[i].skl = nullptr; out[i].flags = 0; out[i].reserved = 0; }
    if (n <= 0) return 0;
    LaneCopies own_stream;                      // (request batches are small: one chunk, this thread)
    return align_on_store(ctx, st, probs, n, out, nullptr, nullptr, nullptr, true, req);
}

// alignS_ng(seqs, pwd, gsi, ori = 3) with seeding off (src/fwd2s1.cc:2746-2760): infer_orientation
// (:2718-2730) scores the query as given and its reverse complement against the opposite strand with
// HomScoreS_ng, keeps the reverse only if it scores strictly higher, then aligns once.
int spdp_align_s_ori3(SpdpContext* ctx, const SpdpScoring* sc, const SpdpProblem* fwd, const SpdpProblem* rev,
                      int n_probs, SpdpAlignment* out, int32_t* orient)
{
    if (!ctx || !sc || !fwd || !rev || !out || !orient) return -1;
    if (n_probs <= 0) return 0;
    std::vector<int32_t> s1(n_probs), s2(n_probs);
    const int r1 = spdp_homscore_s(ctx, sc, fwd, n_probs, s1.data());
    if (r1 < 0) return -1;
    const int r2 = spdp_homscore_s(ctx, sc, rev, n_probs, s2.data());
    if (r2 < 0) return -1;
    std::vector<SpdpProblem> pick(n_probs);
    for (int i = 0; i < n_probs; ++i) {
        orient[i] = s2[i] > s1[i] ? 1 : 0;
        pick[i] = orient[i] ? rev[i] : fwd[i];
    }
    const int r3 = spdp_align_s(ctx, sc, pick.data(), n_probs, out);
    if (r3 < 0) return -1;
    // globalS_ng marks an alignment of the flipped pair: skl->m |= A_RevCom when a->inex.sens is set, which
    // comrev() does (src/fwd2s1.cc:2691-2692, src/aln.h:89)
    for (int i = 0; i < n_probs; ++i)
        if (orient[i] && out[i].skl && out[i].n_skl > 0) out[i].skl[0].m |= 0x10;
    return r1 | r2 | r3;
}
