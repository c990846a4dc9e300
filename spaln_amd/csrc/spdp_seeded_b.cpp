// spdp_seeded_b.cpp -- alignB_ng with seeding on (algmode.qck = 1 .. 3, `spaln -Q1 .. -Q3` on two protein files): the walks of
// a batch of pairs over their HSPs, every DP call of every walk served by the device in common rounds.
//
// What it mirrors (ogotoh/spaln v3.0.7): Aln2b1::globalB_ng -> seededB_ng -> lspB_ng (src/fwd2b1.cc:1531-1560, 1404-1529,
// 1245-1269); the walk itself is spdp_b_seeded_walk.h.  Same scheme as spdp_seeded.cpp / spdp_seeded_h.cpp: the walks run on
// fibers (spdp_seeded_rv.h); a walk that reaches lspB_ng parks its request; the parked requests run as one round on the
// resident residues of the call's pairs (spdp_b_run_requests, spdp_b_api.cpp: the thin sweep for requests of at most 16 rows,
// the tiled sweep for the rest, the branches without a DP cell on the host).  The HSP searches of all levels are the library's
// own (spdp_hsp_host.h with the protein-pair model, the sequences presented with bbt = 1 and lsg = 0 as AvsA sets them,
// src/spaln.cc:713) unless the caller's SpdpHspSource answers them.
#include <atomic>
#include <chrono>
#include <cstring>
#include <mutex>
#include <vector>

#include "spdp_internal.h"
#include "spdp_b_seeded_walk.h"
#include "spdp_hsp_host.h"
#include "spdp_seeded_rv.h"

namespace {
using namespace spdp_seed;

struct DeviceBackendB : DpBackend {
    Fiber* fiber = nullptr; int query = 0;
    const SpdpHspSource* src = nullptr; const SpdpWilipModel* wm = nullptr;
    const SpdpProblem* prob = nullptr; const SpdpScoring* sc = nullptr;
    std::atomic<int64_t>* n_wilip = nullptr;
    bool failed = false, not_computed = false;
    int lsp(const Span& s, const SpdpWindow& w, Records& rec) override
    {
        Parked p;
        p.query = query; p.kind = 0; p.s = s; p.w = w;
        fiber->park(&p);                        // back when the request has been served
        if (p.failed) { failed = true; return SPDP_NEVSEL; }
        if (p.flags) { not_computed = true; return SPDP_NEVSEL; }
        rec.insert(rec.end(), p.rec.begin(), p.rec.end());
        return p.score;
    }
    int trcbk(const Span&, const SpdpWindow&, bool, const int*, Records&) override { failed = true; return SPDP_NEVSEL; }   // (this walk has no such call)
    bool wilip(int level, const Span& s, std::vector<Unit>& units) override
    {
        ++*n_wilip;
        if (src && src->units) {
            const int32_t span[8] = {s.al, s.ar, s.bl, s.br, s.a_exgl, s.a_exgr, s.b_exgl, s.b_exgr};
            const int32_t* flat = nullptr; int32_t n = 0;
            if (src->units(src->user, query, level, span, &flat, &n) || !flat) return false;
            const bool ok = parse_units(flat, n, units);
            if (src->release) src->release(src->user, query, flat);
            return ok;
        }
        if (!wm) return false;
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

extern "C" const char* spdp_align_b_seeded_refusal(const SpdpScoring* sc, const SpdpUnsplicedParams* up, const SpdpSeedParams* sp,
                                                   int hsps_for_all, int has_src)
{
    if (const char* why = spdp_b_refused(sc, up)) return why;
    if (const char* why = seed_params_refused_b(sp, has_src != 0, hsps_for_all != 0)) return why;
    if (((sp->lcl & 16) != 0) != (sc->local != 0)) return "SpdpSeedParams.lcl bit 16 must say what SpdpScoring.local says";
    return nullptr;
}

extern "C" int spdp_align_b_seeded(SpdpContext* ctx, const SpdpScoring* sc, const SpdpUnsplicedParams* up, const SpdpSeedParams* sp,
                                   const SpdpProblem* probs, int n_probs, const SpdpJuxt* const* hsps, const int32_t* n_hsps,
                                   const int32_t* lowest_level, const SpdpHspSource* src, SpdpAlignment* out)
{
    if (!ctx) return -1;
    memset(ctx->seed_stats_b, 0, sizeof ctx->seed_stats_b);
    bool all_bring = n_probs > 0 && hsps && n_hsps;
    for (int i = 0; all_bring && i < n_probs; ++i) all_bring = hsps[i] && n_hsps[i] > 0;
    if (const char* why = spdp_align_b_seeded_refusal(sc, up, sp, all_bring, src && src->units)) { ctx->err = std::string("spdp_align_b_seeded: ") + why; return -1; }
    if (n_probs <= 0) return 0;
    if (!probs || !out) { ctx->err = "spdp_align_b_seeded: null argument"; return -1; }
    for (int i = 0; i < n_probs; ++i) {
        out[i].score = SPDP_NEVSEL; out[i].n_skl = 0; out[i].skl = nullptr; out[i].flags = 0; out[i].reserved = 0;
        if (const char* why = spdp_b_bad_problem(sc, &probs[i])) { ctx->err = "spdp_align_b_seeded: problem " + std::to_string(i) + ": " + why; return -1; }
        const int nh = (hsps && n_hsps && hsps[i]) ? n_hsps[i] : 0;
        for (int j = 0; j < nh; ++j) {
            const SpdpJuxt& h = hsps[i][j];
            if (h.jlen < 0 || h.jx < probs[i].a_left || h.jy < probs[i].b_left || h.jx + h.jlen > probs[i].a_right || h.jy + h.jlen > probs[i].b_right) {
                ctx->err = "spdp_align_b_seeded: problem " + std::to_string(i) + ": an HSP outside the ranges"; return -1;
            }
        }
    }
    const auto t_begin = std::chrono::steady_clock::now();
    auto us_since = [](std::chrono::steady_clock::time_point t) {
        return (int64_t) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t).count(); };
    SpdpBResident resident;
    if (spdp_b_resident_open(ctx, sc, probs, n_probs, &resident)) return -1;

    std::atomic<int64_t> n_wilip{0};
    std::vector<int> scores(n_probs, SPDP_NEVSEL);
    std::vector<Records> recs(n_probs);
    std::vector<uint8_t> status(n_probs, 0);            // 1: an HSP search nobody answered, 2: a request failed, 3: a request above the budget
    auto walk = [&](int q, Fiber& fb) {
        try {                                           // (everything a walk allocates is inside: a walk that throws fails alone)
            DeviceBackendB be;
            be.fiber = &fb; be.query = q; be.src = src; be.wm = sp->wilip; be.prob = &probs[q]; be.sc = sc; be.n_wilip = &n_wilip;
            WalkB w;
            const int nh = (hsps && n_hsps && hsps[q]) ? n_hsps[q] : 0;
            bind_problem_b(w, sc, sp, &probs[q], nh ? hsps[q] : nullptr, nh, lowest_level ? lowest_level[q] : 0);
            w.dp = &be;
            const SpdpProblem& p = probs[q];
            const Span whole = {p.a_left, p.a_right, p.b_left, p.b_right, p.a_exgl, p.a_exgr, p.b_exgl, p.b_exgr};
            scores[q] = w.run(whole);
            recs[q].swap(w.rec);
            status[q] = be.failed ? 2 : (be.not_computed ? 3 : (w.unsupported ? 1 : 0));
        } catch (...) { status[q] = 2; }
    };

    std::atomic<int> rc{0};
    int64_t us_walks = 0, us_device = 0, rstats[SPDP_BREQ_N_STATS] = {0};
    auto t_idle = std::chrono::steady_clock::now();
    auto device = [&](std::vector<Parked*>& take, int) {
        us_walks += us_since(t_idle);
        const auto t0 = std::chrono::steady_clock::now();
        const int m = (int) take.size();
        std::vector<SpdpBRequest> rq(m);
        std::vector<SpdpBRequest*> ptr(m);
        for (int k = 0; k < m; ++k) {
            const Parked& q = *take[k];
            SpdpBRequest& r = rq[k];
            r.parent = q.query;
            r.p = probs[q.query];
            r.p.a_left = q.s.al; r.p.a_right = q.s.ar; r.p.b_left = q.s.bl; r.p.b_right = q.s.br;
            r.p.a_exgl = q.s.a_exgl; r.p.a_exgr = q.s.a_exgr; r.p.b_exgl = q.s.b_exgl; r.p.b_exgr = q.s.b_exgr;
            r.w = q.w;
            ptr[k] = &r;
        }
        const int brc = rc < 0 ? -1 : spdp_b_run_requests(ctx, sc, up, &resident, ptr.data(), m, rstats);
        if (brc < 0) rc = -1;                           // the walks still have to be let go: every request fails from here on
        for (int k = 0; k < m; ++k) {
            Parked& q = *take[k];
            if (brc < 0) { q.failed = true; continue; }
            q.flags = rq[k].status;
            q.score = rq[k].score;
            q.rec.swap(rq[k].rec);
        }
        us_device += us_since(t0);
        t_idle = std::chrono::steady_clock::now();
    };
    WalkScheduler ws;
    ws.all_in_flight = true;                            // a walk's requests are a few rows each: the rounds are bound by their number, not their size
    // the walks of long pairs first: a call ends with its last walk
    ws.order.resize(n_probs);
    for (int i = 0; i < n_probs; ++i) ws.order[i] = i;
    std::stable_sort(ws.order.begin(), ws.order.end(), [&](int x, int y) { return probs[x].a_len + probs[x].b_len > probs[y].a_len + probs[y].b_len; });
    if (!ws.run(n_probs, walk, device, std::vector<int>(1, 0), [](const Parked&) { return 0; })) {
        ctx->err = "spdp_align_b_seeded: could not allocate a stack for a walk"; rc = -1;
    }
    us_walks += us_since(t_idle);
    int64_t* st = ctx->seed_stats_b;
    st[0] = n_probs; st[1] = n_wilip.load(); st[2] = rstats[0]; st[3] = rstats[1]; st[4] = rstats[2]; st[5] = rstats[3];
    st[6] = rstats[4]; st[7] = rstats[5]; st[8] = rstats[6]; st[9] = rstats[7];
    st[10] = us_walks; st[11] = us_device; st[12] = us_since(t_begin);
    if (rc < 0) return -1;

    // globalB_ng's tail (src/fwd2b1.cc:1551-1559): the file without its dummy record -> header + stdskl; no record: no alignment
    int unserved = 0, not_computed = 0;
    for (int i = 0; i < n_probs; ++i) {
        if (status[i] == 3) { ++not_computed; continue; }
        if (status[i]) { ++unserved; continue; }
        out[i].score = scores[i];
        if (recs[i].size() < 2 || scores[i] <= SPDP_NEVSEL) continue;
        const std::vector<SpdpSkl> c = corner_list<1>(std::vector<SpdpSkl>(recs[i].begin() + 1, recs[i].end()));
        out[i].skl = (SpdpSkl*) malloc(sizeof(SpdpSkl) * (c.size() + 1));
        if (!out[i].skl) { ctx->err = "spdp_align_b_seeded: out of memory"; return -1; }
        out[i].skl[0].m = 1; out[i].skl[0].n = (int) c.size();
        std::copy(c.begin(), c.end(), out[i].skl + 1);
        out[i].n_skl = (int) c.size() + 1;
    }
    if (unserved) {
        ctx->err = "spdp_align_b_seeded: " + std::to_string(unserved) + " walk(s) met an HSP search nobody answered or a request that failed; those pairs come back without an alignment";
        return 1;
    }
    if (not_computed) {
        ctx->err = "spdp_align_b_seeded: " + std::to_string(not_computed) + " pair(s) with a request above max_trace_bytes were not computed";
        return 1;
    }
    return 0;
}

extern "C" int spdp_seeded_stats_b(const SpdpContext* ctx, int64_t* out, int n)
{
    if (!ctx || !out) return -1;
    for (int i = 0; i < n && i < 16; ++i) out[i] = ctx->seed_stats_b[i];
    return 0;
}
