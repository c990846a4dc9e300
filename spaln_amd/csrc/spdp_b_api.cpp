// spdp_b_api.cpp -- the unspliced aligner's entries (include/spdp.h "unspliced alignment"): alignB_ng with seeding off
// (globalB_ng -> the direct part of lspB_ng -> trcbkalignB_ng -> stdskl, src/fwd2b1.cc:1104-1148, 1245-1269, 1531-1560),
// HomScoreB_ng under -A0 (scorealoneB_ng), skl_rngB_ng with its edit records on the host, and the rounds of lspB_ng requests on
// resident inputs that the seeded entry asks for (spdp_b_run_requests; spdp_lsp_b: one request per problem, for callers and tests).
//   host:    stripe(), the empty ranges and the one-diagonal window of lspB_ng (no DP cell), the record fix-up, stdskl
//   device:  everything else (spdp_b_forward.hip), in chunks whose traceback stores fit SpdpUnsplicedParams::max_trace_bytes,
//            longest problems first
#include "spdp_internal.h"
#include "spdp_b_dev.h"
#include "spdp_b_host.h"
#include "spdp_b_walk.h"
#include <algorithm>
#include <climits>
#include <cstring>
#include <numeric>
#include <vector>

hipError_t spdp_b_launch(hipStream_t s, bool score, bool dagp, int n, const DevScoringB* sc, const DevProblemB* probs, const uint8_t* codes,
                         int32_t* rowp, int32_t* lastc, uint8_t* trace, int2* recs, DevResultB* res);
hipError_t spdp_b_launch_round(hipStream_t s, bool dagp, int n_wide, int n_thin, const DevScoringB* sc, const DevProblemB* probs,
                               const uint8_t* codes, int32_t* rowp, int32_t* lastc, uint8_t* trace, int2* recs, DevResultB* res);

namespace {

using namespace spdp_bh;
constexpr int64_t DEFAULT_TRACE_BYTES = (int64_t) 4 << 30;

// null: the bundle can be served; otherwise what is wrong with it
const char* refused(const SpdpScoring* sc, const SpdpUnsplicedParams* up)
{
    if (!sc || !up) return "null argument";
    if (sc->spj != 0) return "SpdpScoring.spj must be 0 (the unspliced aligner has no splice terms)";
    if (sc->scalar_engines != 1) return "SpdpScoring.scalar_engines must be 1 (only the -A0 engine of Aln2b1 is reproduced)";
    if (sc->mtx_dim < 1 || sc->mtx_dim > 32) return "SpdpScoring.mtx_dim must be 1 .. 32";
    if (sc->noll != 2 && sc->noll != 3) return "SpdpScoring.noll must be 2 or 3";
    if (up->max_trace_bytes < 0) return "SpdpUnsplicedParams.max_trace_bytes must not be negative";
    return nullptr;
}
const char* bad_problem(const SpdpScoring& sc, const SpdpProblem& p)
{
    if (!p.a || !p.b) return "null sequence";
    if (p.a_left < 0 || p.a_left > p.a_right || p.a_right > p.a_len) return "a range outside the sequence";
    if (p.b_left < 0 || p.b_left > p.b_right || p.b_right > p.b_len) return "b range outside the sequence";
    for (int i = p.a_left; i < p.a_right; ++i) if (p.a[i] >= sc.mtx_dim) return "residue code of a not below mtx_dim";
    for (int i = p.b_left; i < p.b_right; ++i) if (p.b[i] >= sc.mtx_dim) return "residue code of b not below mtx_dim";
    return nullptr;
}

void device_scoring(const SpdpScoring& sc, DevScoringB& hs)
{
    memset(&hs, 0, sizeof hs);
    hs.mtx_dim = sc.mtx_dim; hs.noll = sc.noll; hs.gop = sc.gop; hs.gep = sc.gep; hs.lgop = sc.lgop; hs.lgep = sc.lgep;
    hs.k1 = k1_of(sc); hs.local = sc.local ? 1 : 0;
    for (int x = 1; x < sc.mtx_dim; ++x) for (int y = 1; y < sc.mtx_dim; ++y) hs.mtx[x * 32 + y] = sc.mtx[x * sc.mtx_dim + y];
}

struct Item { int idx; SpdpWindow w; int64_t cells, tbytes; };

// runs one chunk on the device; items in dispatch order.  score mode: scores[idx]; forward: recs[idx] + scores[idx]
int run_chunk(SpdpContext* ctx, const SpdpScoring& sc, const SpdpUnsplicedParams& up, const SpdpProblem* probs, const Item* items, int n,
              bool score, int32_t* scores, std::vector<std::vector<SpdpSkl>>* recs)
{
    DevPool& pool = ctx->pool[B_POOL];
    std::vector<DevProblemB> dp(n);
    int64_t n_codes = 0, n_row = 0, n_col = 0, n_trace = 0, n_rec = 0;
    for (int j = 0; j < n; ++j) {
        const SpdpProblem& p = probs[items[j].idx];
        DevProblemB& d = dp[j];
        memset(&d, 0, sizeof d);
        d.a_off = n_codes; n_codes += p.a_len;
        d.b_off = n_codes; n_codes += p.b_len;
        const int rows = p.a_right - p.a_left, cols = p.b_right - p.b_left;
        d.row_off = n_row; n_row += 3 * (int64_t) (cols + 1);
        d.col_off = n_col; n_col += rows + 1;
        forward_terms(sc, up.tgapf, p, items[j].w, d);
        if (score) {
            d.top = edge(sc, p.a_exgl ? 0.f : 1.f);          // (a global left end of a: the kernel runs sinitB_ng's row itself)
            d.left = edge(sc, p.b_exgl ? 0.f : 1.f);
            d.end_mode = (p.b_exgr ? 1 : 0) | (p.a_exgr ? 2 : 0);
            d.endb = d.enda = DevEdgeB{0, 0, 0};
        } else {
            d.trace_off = n_trace; n_trace += items[j].tbytes;
            d.tstride = (int) tile_stride(p, items[j].w);
            d.rec_cap = (rows + cols) / 2 + 8;
            d.rec_off = n_rec; n_rec += d.rec_cap;
        }
    }
    DevScoringB hs;
    device_scoring(sc, hs);

    auto* d_sc = (DevScoringB*) pool.get(BP_SC, sizeof hs);
    auto* d_probs = (DevProblemB*) pool.get(BP_PROBS, sizeof(DevProblemB) * n);
    auto* d_codes = (uint8_t*) pool.get(BP_CODES, (size_t) n_codes + 4);
    auto* d_rowp = (int32_t*) pool.get(BP_ROWP, sizeof(int32_t) * n_row);
    auto* d_lastc = (int32_t*) pool.get(BP_LASTC, sizeof(int32_t) * n_col);
    auto* d_trace = score ? nullptr : (uint8_t*) pool.get(BP_TRACE, (size_t) n_trace + 4);
    auto* d_recs = score ? nullptr : (int2*) pool.get(BP_RECS, sizeof(int2) * n_rec);
    auto* d_res = (DevResultB*) pool.get(BP_RES, sizeof(DevResultB) * n);
    if (!d_sc || !d_probs || !d_codes || !d_rowp || !d_lastc || !d_res || (!score && (!d_trace || !d_recs))) {
        ctx->err = "unspliced aligner: out of device memory"; return -1;
    }
    std::vector<uint8_t> codes((size_t) n_codes);
    for (int j = 0; j < n; ++j) {
        const SpdpProblem& p = probs[items[j].idx];
        memcpy(codes.data() + dp[j].a_off, p.a, (size_t) p.a_len);
        memcpy(codes.data() + dp[j].b_off, p.b, (size_t) p.b_len);
    }
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(d_sc, &hs, sizeof hs, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_probs, dp.data(), sizeof(DevProblemB) * n, hipMemcpyHostToDevice, s));
    if (n_codes) HIPCHK(hipMemcpyAsync(d_codes, codes.data(), (size_t) n_codes, hipMemcpyHostToDevice, s));
    HIPCHK(spdp_b_launch(s, score, sc.noll == 3, n, d_sc, d_probs, d_codes, d_rowp, d_lastc, d_trace, d_recs, d_res));
    std::vector<DevResultB> res(n);
    HIPCHK(hipMemcpyAsync(res.data(), d_res, sizeof(DevResultB) * n, hipMemcpyDeviceToHost, s));
    std::vector<int2> hrec;
    if (!score) {
        hrec.resize((size_t) n_rec);
        HIPCHK(hipMemcpyAsync(hrec.data(), d_recs, sizeof(int2) * n_rec, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    for (int j = 0; j < n; ++j) {
        const int i = items[j].idx;
        scores[i] = res[j].score;
        if (score) continue;
        if (res[j].n_rec > dp[j].rec_cap) { ctx->err = "unspliced aligner: record list of a problem exceeds its bound"; return -1; }
        std::vector<SpdpSkl>& r = (*recs)[i];
        r.resize(res[j].n_rec);
        for (int k = 0; k < res[j].n_rec; ++k) { r[k].m = hrec[dp[j].rec_off + k].x; r[k].n = hrec[dp[j].rec_off + k].y; }
    }
    return 0;
}

// cuts the device items (sorted longest first) into chunks below the budget and runs them
int run_items(SpdpContext* ctx, const SpdpScoring& sc, const SpdpUnsplicedParams& up, const SpdpProblem* probs, std::vector<Item>& items,
              bool score, int32_t* scores, std::vector<std::vector<SpdpSkl>>* recs)
{
    std::stable_sort(items.begin(), items.end(), [](const Item& x, const Item& y) { return x.cells > y.cells; });
    const int64_t budget = up.max_trace_bytes ? up.max_trace_bytes : DEFAULT_TRACE_BYTES;
    (void) hipSetDevice(ctx->device);
    for (size_t at = 0; at < items.size(); ) {
        size_t end = at;
        int64_t used = 0;
        while (end < items.size() && (score || end == at || used + items[end].tbytes <= budget) && end - at < (size_t) 1 << 20) used += items[end++].tbytes;
        if (run_chunk(ctx, sc, up, probs, items.data() + at, (int) (end - at), score, scores, recs)) return -1;
        at = end;
    }
    return 0;
}

// globalB_ng's tail for one problem: the score, and header {1, corners} + stdskl of the closed records (none: no alignment)
bool hand_over(int score, const std::vector<SpdpSkl>& r, SpdpAlignment& out)
{
    out.score = score;
    if (r.empty() || score <= SPDP_NEVSEL) return true;
    const std::vector<SpdpSkl> c = corner_list<1>(r);
    out.skl = (SpdpSkl*) malloc(sizeof(SpdpSkl) * (c.size() + 1));
    if (!out.skl) return false;
    out.skl[0].m = 1; out.skl[0].n = (int) c.size();
    std::copy(c.begin(), c.end(), out.skl + 1);
    out.n_skl = (int) c.size() + 1;
    return true;
}

}   // namespace

const char* spdp_b_refused(const SpdpScoring* sc, const SpdpUnsplicedParams* up) { return refused(sc, up); }
const char* spdp_b_bad_problem(const SpdpScoring* sc, const SpdpProblem* p) { return bad_problem(*sc, *p); }

// ---- requests on resident inputs (spdp_internal.h)
int spdp_b_resident_open(SpdpContext* ctx, const SpdpScoring* sc, const SpdpProblem* probs, int n, SpdpBResident* res)
{
    res->a_off.assign(n, 0); res->b_off.assign(n, 0);
    int64_t n_codes = 0;
    for (int i = 0; i < n; ++i) { res->a_off[i] = n_codes; n_codes += probs[i].a_len; res->b_off[i] = n_codes; n_codes += probs[i].b_len; }
    std::vector<uint8_t> codes((size_t) n_codes);
    for (int i = 0; i < n; ++i) {
        memcpy(codes.data() + res->a_off[i], probs[i].a, (size_t) probs[i].a_len);
        memcpy(codes.data() + res->b_off[i], probs[i].b, (size_t) probs[i].b_len);
    }
    DevScoringB hs;
    device_scoring(*sc, hs);
    (void) hipSetDevice(ctx->device);
    DevPool& pool = ctx->pool[B_POOL];
    auto* d_sc = (DevScoringB*) pool.get(BP_SC, sizeof hs);
    auto* d_codes = (uint8_t*) pool.get(BP_RESIDENT, (size_t) n_codes + 4);
    if (!d_sc || !d_codes) { ctx->err = "unspliced aligner: out of device memory"; return -1; }
    HIPCHK(hipMemcpyAsync(d_sc, &hs, sizeof hs, hipMemcpyHostToDevice, ctx->stream));
    if (n_codes) HIPCHK(hipMemcpyAsync(d_codes, codes.data(), (size_t) n_codes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

namespace {

struct RoundItem { SpdpBRequest* r; bool thin; int64_t cells, tbytes; int steps; };

// one launch set: items[0 .. n_wide) tiled, the rest thin
int run_round(SpdpContext* ctx, const SpdpScoring& sc, const SpdpUnsplicedParams& up, const SpdpBResident& rs, const RoundItem* items, int n_wide, int n_thin)
{
    const int n = n_wide + n_thin;
    DevPool& pool = ctx->pool[B_POOL];
    std::vector<DevProblemB> dp(n);
    int64_t n_row = 0, n_col = 0, n_trace = 0, n_rec = 0;
    for (int j = 0; j < n; ++j) {
        const SpdpBRequest& q = *items[j].r;
        const SpdpProblem& p = q.p;
        DevProblemB& d = dp[j];
        memset(&d, 0, sizeof d);
        d.a_off = rs.a_off[q.parent]; d.b_off = rs.b_off[q.parent];
        const int rows = p.a_right - p.a_left, cols = p.b_right - p.b_left;
        d.row_off = n_row; n_row += (items[j].thin ? 1 : 3) * (int64_t) (cols + 1);
        d.col_off = n_col; n_col += rows + 1;
        forward_terms(sc, up.tgapf, p, q.w, d);
        d.thin = items[j].thin ? 1 : 0;
        d.trace_off = n_trace; n_trace += items[j].tbytes;
        d.tstride = items[j].thin ? 0 : (int) tile_stride(p, q.w);
        d.rec_cap = (rows + cols) / 2 + 8;
        d.rec_off = n_rec; n_rec += d.rec_cap;
    }
    auto* d_sc = (DevScoringB*) pool.get(BP_SC, sizeof(DevScoringB));
    auto* d_codes = (uint8_t*) pool.ptr[BP_RESIDENT];
    auto* d_probs = (DevProblemB*) pool.get(BP_PROBS, sizeof(DevProblemB) * n);
    auto* d_rowp = (int32_t*) pool.get(BP_ROWP, sizeof(int32_t) * n_row);
    auto* d_lastc = (int32_t*) pool.get(BP_LASTC, sizeof(int32_t) * n_col);
    auto* d_trace = (uint8_t*) pool.get(BP_TRACE, (size_t) n_trace + 4);
    auto* d_recs = (int2*) pool.get(BP_RECS, sizeof(int2) * n_rec);
    auto* d_res = (DevResultB*) pool.get(BP_RES, sizeof(DevResultB) * n);
    if (!d_sc || !d_codes || !d_probs || !d_rowp || !d_lastc || !d_trace || !d_recs || !d_res) { ctx->err = "unspliced aligner: out of device memory"; return -1; }
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(d_probs, dp.data(), sizeof(DevProblemB) * n, hipMemcpyHostToDevice, s));
    HIPCHK(spdp_b_launch_round(s, sc.noll == 3, n_wide, n_thin, d_sc, d_probs, d_codes, d_rowp, d_lastc, d_trace, d_recs, d_res));
    std::vector<DevResultB> res(n);
    std::vector<int2> hrec((size_t) n_rec);
    HIPCHK(hipMemcpyAsync(res.data(), d_res, sizeof(DevResultB) * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hrec.data(), d_recs, sizeof(int2) * n_rec, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int j = 0; j < n; ++j) {
        SpdpBRequest& q = *items[j].r;
        q.score = res[j].score;
        if (res[j].n_rec > dp[j].rec_cap) { ctx->err = "unspliced aligner: record list of a request exceeds its bound"; return -1; }
        q.rec.resize(res[j].n_rec);
        for (int k = 0; k < res[j].n_rec; ++k) { q.rec[k].m = hrec[dp[j].rec_off + k].x; q.rec[k].n = hrec[dp[j].rec_off + k].y; }
        close_records(sc, q.p, q.rec);
    }
    return 0;
}

}   // namespace

int spdp_b_run_requests(SpdpContext* ctx, const SpdpScoring* sc, const SpdpUnsplicedParams* up, const SpdpBResident* rs,
                        SpdpBRequest* const* reqs, int n, int64_t* stats)
{
    const int64_t budget = up->max_trace_bytes ? up->max_trace_bytes : DEFAULT_TRACE_BYTES;
    const bool thin_on = spdp_knob_on("SPDP_B_THIN");
    // SPDP_B_THIN_SORT=0: the thin requests run in the order given, so that a caller (the tests) decides which four share a
    // wave and in which slot the longest of them sits; the kernel does not depend on the order
    const bool thin_sorted = spdp_knob_on("SPDP_B_THIN_SORT");
    std::vector<RoundItem> items;
    for (int i = 0; i < n; ++i) {
        SpdpBRequest& q = *reqs[i];
        q.status = 0; q.rec.clear(); q.score = SPDP_NEVSEL;
        if (lsp_without_cells(*sc, q.p, q.w, q.score, q.rec)) { ++stats[3]; continue; }
        const int rows = q.p.a_right - q.p.a_left;
        RoundItem it = {&q, thin_on && rows <= 16, spdp_cells_b(&q.p, &q.w), 0, 0};
        DevProblemB d;
        memset(&d, 0, sizeof d);
        forward_terms(*sc, up->tgapf, q.p, q.w, d);
        const ThinGeoB g = thin_geo_b(d);
        it.steps = g.steps;
        it.tbytes = it.thin ? thin_trace_bytes_b(d) : trace_bytes(q.p, q.w);
        stats[6] += it.cells;
        if (rows <= 16) { ++stats[4]; stats[5] += it.cells; }
        if (it.tbytes > budget) { q.status = 1; ++stats[7]; continue; }
        ++stats[it.thin ? 1 : 2];
        items.push_back(it);
    }
    // tiled requests longest first, then the thin ones by step count, so that the four of a wave are alike
    std::stable_sort(items.begin(), items.end(), [thin_sorted](const RoundItem& x, const RoundItem& y) {
        if (x.thin != y.thin) return !x.thin;
        return x.thin ? (thin_sorted && x.steps > y.steps) : x.cells > y.cells; });
    (void) hipSetDevice(ctx->device);
    for (size_t at = 0; at < items.size(); ) {
        size_t end = at;
        int64_t used = 0;
        while (end < items.size() && (end == at || used + items[end].tbytes <= budget) && end - at < (size_t) 1 << 20) used += items[end++].tbytes;
        int n_wide = 0;
        for (size_t j = at; j < end; ++j) n_wide += !items[j].thin;
        if (run_round(ctx, *sc, *up, *rs, items.data() + at, n_wide, (int) (end - at) - n_wide)) return -1;
        ++stats[0];
        at = end;
    }
    return 0;
}

extern "C" int64_t spdp_cells_b(const SpdpProblem* p, const SpdpWindow* w)
{
    if (!p || !w) return 0;
    int64_t c = 0;
    for (int m = p->a_left + 1; m <= p->a_right; ++m) {
        const int lo = std::max(m - 1 + w->lw, p->b_left), hi = std::min(m + w->up, p->b_right);
        if (hi > lo) c += hi - lo;
    }
    return c;
}

extern "C" int64_t spdp_trace_bytes_b(const SpdpProblem* p, const SpdpWindow* w)
{
    if (!p || !w || p->a_right <= p->a_left || p->b_right <= p->b_left || w->up <= w->lw) return 0;
    return trace_bytes(*p, *w);
}

extern "C" int spdp_align_b(SpdpContext* ctx, const SpdpScoring* sc, const SpdpUnsplicedParams* up, const SpdpProblem* probs, int n,
                            SpdpAlignment* out)
{
    if (!ctx) return -1;
    if (const char* why = refused(sc, up)) { ctx->err = std::string("spdp_align_b: ") + why; return -1; }
    if (n <= 0) return 0;
    if (!probs || !out) { ctx->err = "spdp_align_b: null argument"; return -1; }
    for (int i = 0; i < n; ++i) {
        out[i].score = SPDP_NEVSEL; out[i].n_skl = 0; out[i].skl = nullptr; out[i].flags = 0; out[i].reserved = 0;
        if (const char* why = bad_problem(*sc, probs[i])) { ctx->err = "spdp_align_b: problem " + std::to_string(i) + ": " + why; return -1; }
    }
    const int64_t budget = up->max_trace_bytes ? up->max_trace_bytes : DEFAULT_TRACE_BYTES;
    std::vector<std::vector<SpdpSkl>> recs(n);
    std::vector<int32_t> scores(n, SPDP_NEVSEL);
    std::vector<Item> items;
    int not_computed = 0;
    for (int i = 0; i < n; ++i) {
        const SpdpProblem& p = probs[i];
        SpdpWindow w;
        spdp_stripe(&p, sc->sh, &w);
        if (lsp_without_cells(*sc, p, w, scores[i], recs[i])) continue;
        Item it = {i, w, spdp_cells_b(&p, &w), trace_bytes(p, w)};
        if (it.tbytes > budget) { ++not_computed; continue; }
        items.push_back(it);
    }
    std::vector<bool> on_device(n, false);
    for (const Item& it : items) on_device[it.idx] = true;
    if (run_items(ctx, *sc, *up, probs, items, false, scores.data(), &recs)) return -1;
    for (int i = 0; i < n; ++i) {
        const SpdpProblem& p = probs[i];
        std::vector<SpdpSkl>& r = recs[i];
        if (on_device[i]) close_records(*sc, p, r);
        if (!hand_over(scores[i], r, out[i])) { ctx->err = "spdp_align_b: out of memory"; return -1; }
    }
    if (not_computed) ctx->err = "spdp_align_b: " + std::to_string(not_computed) + " problem(s) above max_trace_bytes were not computed";
    return not_computed ? 1 : 0;
}

extern "C" int spdp_lsp_b(SpdpContext* ctx, const SpdpScoring* sc, const SpdpUnsplicedParams* up, const SpdpProblem* probs, int n,
                          SpdpAlignment* out, int64_t* stats)
{
    if (!ctx) return -1;
    if (stats) memset(stats, 0, sizeof(int64_t) * SPDP_BREQ_N_STATS);
    if (const char* why = refused(sc, up)) { ctx->err = std::string("spdp_lsp_b: ") + why; return -1; }
    if (n <= 0) return 0;
    if (!probs || !out) { ctx->err = "spdp_lsp_b: null argument"; return -1; }
    for (int i = 0; i < n; ++i) {
        out[i].score = SPDP_NEVSEL; out[i].n_skl = 0; out[i].skl = nullptr; out[i].flags = 0; out[i].reserved = 0;
        if (const char* why = bad_problem(*sc, probs[i])) { ctx->err = "spdp_lsp_b: problem " + std::to_string(i) + ": " + why; return -1; }
    }
    SpdpBResident resident;
    if (spdp_b_resident_open(ctx, sc, probs, n, &resident)) return -1;
    std::vector<SpdpBRequest> rq(n);
    std::vector<SpdpBRequest*> ptr(n);
    for (int i = 0; i < n; ++i) {
        rq[i].parent = i;
        rq[i].p = probs[i];
        // the walk's window of a request is ladder::stripe<1> on the request's ranges (spdp_b_seeded_walk.h); spdp_stripe is
        // that very function on the problem's ranges (spdp_api.cpp)
        spdp_stripe(&probs[i], sc->sh, &rq[i].w);
        ptr[i] = &rq[i];
    }
    int64_t st[SPDP_BREQ_N_STATS] = {0};
    if (spdp_b_run_requests(ctx, sc, up, &resident, ptr.data(), n, st)) return -1;
    if (stats) memcpy(stats, st, sizeof st);
    int not_computed = 0;
    for (int i = 0; i < n; ++i) {
        if (rq[i].status) { ++not_computed; continue; }
        if (!hand_over(rq[i].score, rq[i].rec, out[i])) { ctx->err = "spdp_lsp_b: out of memory"; return -1; }
    }
    if (not_computed) ctx->err = "spdp_lsp_b: " + std::to_string(not_computed) + " request(s) above max_trace_bytes were not computed";
    return not_computed ? 1 : 0;
}

extern "C" int spdp_homscore_b(SpdpContext* ctx, const SpdpScoring* sc, const SpdpUnsplicedParams* up, const SpdpProblem* probs, int n,
                               int32_t* scores)
{
    if (!ctx) return -1;
    if (const char* why = refused(sc, up)) { ctx->err = std::string("spdp_homscore_b: ") + why; return -1; }
    if (n <= 0) return 0;
    if (!probs || !scores) { ctx->err = "spdp_homscore_b: null argument"; return -1; }
    std::vector<Item> items;
    for (int i = 0; i < n; ++i) {
        if (const char* why = bad_problem(*sc, probs[i])) { ctx->err = "spdp_homscore_b: problem " + std::to_string(i) + ": " + why; return -1; }
        SpdpWindow w;
        spdp_stripe(&probs[i], sc->sh, &w);
        scores[i] = SPDP_NEVSEL;
        if (w.width < 3) continue;
        items.push_back({i, w, spdp_cells_b(&probs[i], &w), 0});
    }
    return run_items(ctx, *sc, *up, probs, items, true, scores, nullptr);
}

namespace {

struct RescoreOut { SpdpRescoredB st; std::vector<SpdpEdit> ed; int sam[5] = {0, 0, 0, 0, 0}; };

// skl_rngB_ng (src/fwd2b1.cc:295-395) over header + corners
void rescore_b(const SpdpScoring& sc, const SpdpUnsplicedParams& up, const SpdpProblem& p, const SpdpAlignment& aln, int format, RescoreOut& o)
{
    memset(&o.st, 0, sizeof o.st);
    if (aln.n_skl < 3 || !aln.skl) return;
    std::vector<SpdpSkl> c(aln.skl + 1, aln.skl + aln.n_skl);
    const SpdpSkl first = c[0];
    trim_skl_of(c, p);
    o.st.first = 1 + ((c[0].m != first.m || c[0].n != first.n) ? 1 : 0);
    o.st.n_trim = (int) c.size();
    auto push = [&](int op, int x, int y) { o.ed.push_back({op, x, y}); };
    int m = c[0].m, n = c[0].n, scr = 0, span = 0;
    if (format == SPDP_FMT_SAM) {
        o.sam[1] = n; o.sam[3] = m;
        if (m) push('H', m, 0);
    }
    float tg = (m == 0 || n == 0) ? up.tgapf : 1.f;
    for (size_t q = 1; q < c.size(); ++q) {
        const int mi = c[q].m - m, ni = c[q].n - n, i = mi - ni;
        int d = i >= 0 ? ni : mi;
        span += std::max(mi, ni);
        if (d) {
            if (format == SPDP_FMT_VULGAR) push('M', d, d); else if (format) push('M', d, 0);
            for (int k = 0; k < d; ++k) {
                const int x = p.a[m + k], y = p.b[n + k];
                scr += sim(sc, x, y);
                if (x == y) ++o.st.mch; else ++o.st.mmc;
            }
            m += d; n += d;
        }
        if (i < 0) { d = -i; if (format == SPDP_FMT_VULGAR) push('G', 0, d); else if (format) push('D', d, 0); }
        else if (i > 0) { d = i; if (format == SPDP_FMT_VULGAR) push('G', d, 0); else if (format) push('I', d, 0); }
        else d = 0;
        if (d) {
            if (c[q].m == p.a_len || c[q].n == p.b_len) tg = up.tgapf;
            o.st.gap += tg;
            o.st.unp += d * tg;
            scr += (int) (gap_penalty(sc, d) * tg);
            tg = 1.f;
        }
        m = c[q].m; n = c[q].n;
    }
    if (format == SPDP_FMT_SAM) {
        if (m < p.a_len) push('H', p.a_len - m, 0);
        o.sam[4] = m;
        o.sam[2] = 30 + (int) (100 * (o.st.mmc + o.st.unp) / p.a_len);
    }
    o.st.val = scr;
    o.st.span = span;
}

const char* rescore_refused(const SpdpScoring* sc, const SpdpUnsplicedParams* up, const SpdpProblem* probs, const SpdpAlignment* aln, int n)
{
    if (const char* why = refused(sc, up)) return why;
    if (n > 0 && (!probs || !aln)) return "null argument";
    for (int i = 0; i < n; ++i) {
        if (bad_problem(*sc, probs[i])) return "bad problem";
        for (int k = 1; k < aln[i].n_skl; ++k)
            if (aln[i].skl[k].m < 0 || aln[i].skl[k].m > probs[i].a_len || aln[i].skl[k].n < 0 || aln[i].skl[k].n > probs[i].b_len ||
                (k > 1 && (aln[i].skl[k].m < aln[i].skl[k - 1].m || aln[i].skl[k].n < aln[i].skl[k - 1].n))) return "corner outside the sequences or out of order";
    }
    return nullptr;
}

}   // namespace

extern "C" int spdp_skl_rng_b(const SpdpScoring* sc, const SpdpUnsplicedParams* up, const SpdpProblem* probs, int n, const SpdpAlignment* aln,
                              SpdpRescoredB* out)
{
    if (rescore_refused(sc, up, probs, aln, n) || (n > 0 && !out)) return -1;
    for (int i = 0; i < n; ++i) {
        RescoreOut o;
        rescore_b(*sc, *up, probs[i], aln[i], 0, o);
        out[i] = o.st;
    }
    return 0;
}

extern "C" int spdp_skl_edits_b(const SpdpScoring* sc, const SpdpUnsplicedParams* up, const SpdpProblem* probs, int n, const SpdpAlignment* aln,
                                int format, SpdpEdits* out)
{
    if (rescore_refused(sc, up, probs, aln, n) || (n > 0 && !out)) return -1;
    if (format != SPDP_FMT_CIGAR && format != SPDP_FMT_VULGAR && format != SPDP_FMT_SAM) return -1;
    for (int i = 0; i < n; ++i) {
        RescoreOut o;
        rescore_b(*sc, *up, probs[i], aln[i], format, o);
        memset(&out[i], 0, sizeof out[i]);
        out[i].n = (int) o.ed.size();
        if (out[i].n) {
            out[i].rec = (SpdpEdit*) malloc(sizeof(SpdpEdit) * o.ed.size());
            if (!out[i].rec) return -1;
            std::copy(o.ed.begin(), o.ed.end(), out[i].rec);
        }
        out[i].sam_flag = o.sam[0]; out[i].sam_pos = o.sam[1]; out[i].sam_mapq = o.sam[2]; out[i].sam_left = o.sam[3]; out[i].sam_right = o.sam[4];
    }
    return 0;
}
