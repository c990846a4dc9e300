// spdp_group.cpp -- several GPUs of one node behind one handle (include/spdp.h, "device groups").
//
// The reference is one multi-threaded process (spaln -t N: a master hands whole queries to worker threads,
// src/spaln.cc:1389-1468); the drop-in counterpart is one process that owns every GPU of the node.  A group
// holds one context per device; a batched call shards the query list by DP cells (longest-processing-time rule;
// problems are independent, SURVEY.md 8e: no data-path exchange, no collective), runs every shard on its own device
// from its own host thread, and the results land in the caller's arrays in query order.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include "../../include/spdp.h"
#include "spdp_internal.h"
#include "spdp_group_gather.h"

struct SpdpGroup {
    std::vector<SpdpContext*> ctx;
    std::string err;
    std::vector<int> shard_of;          // member that ran problem i in the last call (spdp_group_last_shards)
};

namespace {
// cost-balanced shards (longest-processing-time rule over the DP cells of every problem; the rule of
// spaln_amd/shard.py: balanced_shards): windows differ by a factor of two and more, and the slowest member bounds the
// call.  idx[r] = the problems of member r, in caller order.
std::vector<std::vector<int>> balanced(const std::vector<int64_t>& cost, int w)
{
    std::vector<int> order(cost.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int) i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cost[x] > cost[y]; });
    std::vector<int64_t> load(w, 0);
    std::vector<std::vector<int>> idx(w);
    for (int i : order) {
        int r = 0;
        for (int k = 1; k < w; ++k) if (load[k] < load[r]) r = k;
        idx[r].push_back(i);
        load[r] += cost[i];
    }
    for (auto& v : idx) std::sort(v.begin(), v.end());
    return idx;
}

// P = SpdpProblem / SpdpProblemH, R = the per-problem result type: member r gets its problems gathered into one array
template <typename P, typename R, typename F>
int fan_out(SpdpGroup* g, const P* probs, int n, const std::vector<int64_t>& cost, R* res, F&& call)
{
    if (!g || g->ctx.empty()) return -1;
    const int w = (int) g->ctx.size();
    const std::vector<std::vector<int>> idx = balanced(cost, w);
    g->shard_of.assign(n, 0);
    std::vector<int> rc(w, 0);
    std::vector<std::thread> th;
    for (int r = 0; r < w; ++r) {
        if (idx[r].empty()) continue;
        for (int i : idx[r]) g->shard_of[i] = r;
        th.emplace_back([&, r]() {
            (void) hipSetDevice(g->ctx[r]->device);
            const int cnt = (int) idx[r].size();
            std::vector<P> mine(cnt);
            std::vector<R> out(cnt);
            for (int k = 0; k < cnt; ++k) { mine[k] = probs[idx[r][k]]; out[k] = res[idx[r][k]]; }
            rc[r] = call(g->ctx[r], mine.data(), cnt, out.data());
            for (int k = 0; k < cnt; ++k) res[idx[r][k]] = out[k];
        });
    }
    for (std::thread& t : th) t.join();
    int worst = 0;
    for (int r = 0; r < w; ++r) {
        if (rc[r] < 0) { g->err = "device " + std::to_string(g->ctx[r]->device) + ": " + g->ctx[r]->err; return -1; }
        worst |= rc[r];
    }
    return worst;
}
}   // namespace

extern "C" {

SpdpGroup* spdp_group_create(const int* devices, int n_devices)
{
    if (!devices || n_devices <= 0) return nullptr;
    SpdpGroup* g = new SpdpGroup();
    for (int i = 0; i < n_devices; ++i) {
        SpdpContext* c = spdp_create(devices[i]);
        if (!c) { spdp_group_destroy(g); return nullptr; }
        g->ctx.push_back(c);
    }
    return g;
}

void spdp_group_destroy(SpdpGroup* g)
{
    if (!g) return;
    for (SpdpContext* c : g->ctx) spdp_destroy(c);
    delete g;
}

int spdp_group_size(const SpdpGroup* g) { return g ? (int) g->ctx.size() : 0; }
const char* spdp_group_last_error(const SpdpGroup* g) { return g ? g->err.c_str() : "null group"; }

static std::vector<int64_t> costs_s(const SpdpScoring* sc, const SpdpProblem* probs, int n)
{
    std::vector<int64_t> c(std::max(n, 0));
    for (int i = 0; i < n; ++i) { SpdpWindow w; spdp_stripe(&probs[i], sc->sh, &w); c[i] = spdp_cells(&probs[i], &w); }
    return c;
}
static std::vector<int64_t> costs_h(const SpdpScoringH* sc, const SpdpProblemH* probs, int n)
{
    std::vector<int64_t> c(std::max(n, 0));
    for (int i = 0; i < n; ++i) { SpdpWindow w; spdp_stripe31(&probs[i], sc->sh, &w); c[i] = spdp_cells_h(&probs[i], &w); }
    return c;
}

int spdp_group_homscore_s(SpdpGroup* g, const SpdpScoring* sc, const SpdpProblem* probs, int n_probs, int32_t* scores)
{
    return fan_out(g, probs, n_probs, costs_s(sc, probs, n_probs), scores, [=](SpdpContext* c, const SpdpProblem* p, int cnt, int32_t* o) {
        return spdp_homscore_s(c, sc, p, cnt, o);
    });
}

int spdp_group_align_s(SpdpGroup* g, const SpdpScoring* sc, const SpdpProblem* probs, int n_probs, SpdpAlignment* out)
{
    return fan_out(g, probs, n_probs, costs_s(sc, probs, n_probs), out, [=](SpdpContext* c, const SpdpProblem* p, int cnt, SpdpAlignment* o) {
        return spdp_align_s(c, sc, p, cnt, o);
    });
}

int spdp_group_homscore_h(SpdpGroup* g, const SpdpScoringH* sc, const SpdpProblemH* probs, int n_probs, int32_t* scores)
{
    return fan_out(g, probs, n_probs, costs_h(sc, probs, n_probs), scores, [=](SpdpContext* c, const SpdpProblemH* p, int cnt, int32_t* o) {
        return spdp_homscore_h(c, sc, p, cnt, o);
    });
}

int spdp_group_align_h(SpdpGroup* g, const SpdpScoringH* sc, const SpdpProblemH* probs, int n_probs, SpdpAlignment* out)
{
    return fan_out(g, probs, n_probs, costs_h(sc, probs, n_probs), out, [=](SpdpContext* c, const SpdpProblemH* p, int cnt, SpdpAlignment* o) {
        return spdp_align_h(c, sc, p, cnt, o);
    });
}

// ---- the calls round 3 / 4 added: seeded alignment, rescoring, the block vote -------------------------------------------
extern "C++" {
namespace {
// a member's HSP source: the caller's, asked with the CALLER's query numbers
struct RemapSource { const SpdpHspSource* src; const int* idx; };
int remap_units(void* user, int32_t query, int32_t level, const int32_t span[8], const int32_t** flat, int32_t* n_flat)
{
    const RemapSource* r = (const RemapSource*) user;
    return r->src->units(r->src->user, r->idx[query], level, span, flat, n_flat);
}
void remap_release(void* user, int32_t query, const int32_t* flat)
{
    const RemapSource* r = (const RemapSource*) user;
    if (r->src->release) r->src->release(r->src->user, r->idx[query], flat);
}

// member r runs call(ctx, its problem numbers in caller order); results are written by the call itself (it knows the layout)
template <typename F>
int fan_out_idx(SpdpGroup* g, int n, const std::vector<int64_t>& cost, F&& call)
{
    if (!g || g->ctx.empty()) return -1;
    const int w = (int) g->ctx.size();
    const std::vector<std::vector<int>> idx = balanced(cost, w);
    g->shard_of.assign(n, 0);
    std::vector<int> rc(w, 0);
    std::vector<std::thread> th;
    for (int r = 0; r < w; ++r) {
        if (idx[r].empty()) continue;
        for (int i : idx[r]) g->shard_of[i] = r;
        th.emplace_back([&, r]() { (void) hipSetDevice(g->ctx[r]->device); rc[r] = call(g->ctx[r], idx[r]); });
    }
    for (std::thread& t : th) t.join();
    int worst = 0;
    for (int r = 0; r < w; ++r) {
        if (rc[r] < 0) { g->err = "device " + std::to_string(g->ctx[r]->device) + ": " + g->ctx[r]->err; return -1; }
        worst |= rc[r];
    }
    return worst;
}

template <typename SC, typename P, typename CALL>
int group_seeded(SpdpGroup* g, const SC* sc, const P* probs, int n, const std::vector<int64_t>& cost,
                 const SpdpJuxt* const* hsps, const int32_t* n_hsps, const int32_t* lowest_level, const SpdpHspSource* src,
                 SpdpAlignment* out, CALL&& call)
{
    return fan_out_idx(g, n, cost, [&](SpdpContext* c, const std::vector<int>& idx) {
        const int cnt = (int) idx.size();
        std::vector<P> mine(cnt);
        std::vector<const SpdpJuxt*> h(cnt);
        std::vector<int32_t> nh(cnt), ll(cnt);
        std::vector<SpdpAlignment> o(cnt);
        for (int k = 0; k < cnt; ++k) {
            mine[k] = probs[idx[k]];
            h[k] = hsps ? hsps[idx[k]] : nullptr;
            nh[k] = n_hsps ? n_hsps[idx[k]] : 0;
            ll[k] = lowest_level ? lowest_level[idx[k]] : 0;
        }
        RemapSource rs = {src, idx.data()};
        SpdpHspSource local = {&rs, remap_units, remap_release};
        const int rc = call(c, sc, mine.data(), cnt, hsps ? h.data() : nullptr, n_hsps ? nh.data() : nullptr,
                            lowest_level ? ll.data() : nullptr, src ? &local : nullptr, o.data());
        for (int k = 0; k < cnt; ++k) out[idx[k]] = o[k];
        return rc;
    });
}
}   // namespace
}   // extern "C++"

// alignS_ng / alignH_ng with seeding on for a batch, sharded over the group's devices by DP cells of the whole windows (the
// reference's counterpart: the -t N master / worker loop, src/spaln.cc:1389-1468); every member runs its own fiber scheduler
// and dispatcher lanes; the HSP source is asked with the caller's query numbers
int spdp_group_align_s_seeded(SpdpGroup* g, const SpdpScoring* sc, const SpdpSeedParams* sp, const SpdpProblem* probs, int n_probs,
                              const SpdpJuxt* const* hsps, const int32_t* n_hsps, const int32_t* lowest_level,
                              const SpdpHspSource* src, SpdpAlignment* out)
{
    return group_seeded(g, sc, probs, n_probs, costs_s(sc, probs, n_probs), hsps, n_hsps, lowest_level, src, out,
                        [=](SpdpContext* c, const SpdpScoring* s, const SpdpProblem* p, int cnt, const SpdpJuxt* const* h, const int32_t* nh,
                            const int32_t* ll, const SpdpHspSource* so, SpdpAlignment* o) { return spdp_align_s_seeded(c, s, sp, p, cnt, h, nh, ll, so, o); });
}
int spdp_group_align_h_seeded(SpdpGroup* g, const SpdpScoringH* sc, const SpdpSeedParams* sp, const SpdpProblemH* probs, int n_probs,
                              const SpdpJuxt* const* hsps, const int32_t* n_hsps, const int32_t* lowest_level,
                              const SpdpHspSource* src, SpdpAlignment* out)
{
    return group_seeded(g, sc, probs, n_probs, costs_h(sc, probs, n_probs), hsps, n_hsps, lowest_level, src, out,
                        [=](SpdpContext* c, const SpdpScoringH* s, const SpdpProblemH* p, int cnt, const SpdpJuxt* const* h, const int32_t* nh,
                            const int32_t* ll, const SpdpHspSource* so, SpdpAlignment* o) { return spdp_align_h_seeded(c, s, sp, p, cnt, h, nh, ll, so, o); });
}

// skl_rngS_ng / skl_rngH_ng for a batch of alignments, sharded by alignment length (records)
int spdp_group_skl_rng_s(SpdpGroup* g, const SpdpScoring* sc, const SpdpRescoreParams* rp, const SpdpProblem* probs, int n_probs,
                         const SpdpAlignment* aln, SpdpRescored* out)
{
    std::vector<int64_t> cost(std::max(n_probs, 0));
    for (int i = 0; i < n_probs; ++i) cost[i] = 1 + std::max(aln[i].n_skl, 0) + (probs[i].a_right - probs[i].a_left);
    return fan_out_idx(g, n_probs, cost, [&](SpdpContext* c, const std::vector<int>& idx) {
        const int cnt = (int) idx.size();
        std::vector<SpdpProblem> mine(cnt);
        std::vector<SpdpAlignment> al(cnt);
        std::vector<SpdpRescored> o(cnt);
        for (int k = 0; k < cnt; ++k) { mine[k] = probs[idx[k]]; al[k] = aln[idx[k]]; o[k] = out[idx[k]]; }
        const int rc = spdp_skl_rng_s(c, sc, rp, mine.data(), cnt, al.data(), o.data());
        for (int k = 0; k < cnt; ++k) out[idx[k]] = o[k];
        return rc;
    });
}
int spdp_group_skl_rng_h(SpdpGroup* g, const SpdpScoringH* sc, const SpdpRescoreParamsH* rp, const SpdpProblemH* probs, int n_probs,
                         const SpdpAlignment* aln, SpdpRescored* out)
{
    std::vector<int64_t> cost(std::max(n_probs, 0));
    for (int i = 0; i < n_probs; ++i) cost[i] = 1 + std::max(aln[i].n_skl, 0) + (probs[i].a_right - probs[i].a_left);
    return fan_out_idx(g, n_probs, cost, [&](SpdpContext* c, const std::vector<int>& idx) {
        const int cnt = (int) idx.size();
        std::vector<SpdpProblemH> mine(cnt);
        std::vector<SpdpAlignment> al(cnt);
        std::vector<SpdpRescored> o(cnt);
        for (int k = 0; k < cnt; ++k) { mine[k] = probs[idx[k]]; al[k] = aln[idx[k]]; o[k] = out[idx[k]]; }
        const int rc = spdp_skl_rng_h(c, sc, rp, mine.data(), cnt, al.data(), o.data());
        for (int k = 0; k < cnt; ++k) out[idx[k]] = o[k];
        return rc;
    });
}

// the block vote for a batch of queries: every member holds its own copy of the index (ix[r] created on the group's r-th
// context: spdp_group_context), the queries are sharded by length
SpdpContext* spdp_group_context(SpdpGroup* g, int member) { return (g && member >= 0 && member < (int) g->ctx.size()) ? g->ctx[member] : nullptr; }
int spdp_group_blk_vote(SpdpGroup* g, const SpdpBlkIndex* const* ix, const uint8_t* codes, const int64_t* offs,
                        const int32_t* left, const int32_t* right, const int32_t* stop_at, int32_t n, int32_t* out, int32_t out_cap)
{
    if (!ix || !codes || !offs || !left || !right || !out) { if (g) g->err = "spdp_group_blk_vote: null argument"; return -1; }
    std::vector<int64_t> cost(std::max(n, 0));
    for (int i = 0; i < n; ++i) cost[i] = 1 + right[i] - left[i];
    return fan_out_idx(g, n, cost, [&](SpdpContext* c, const std::vector<int>& idx) {
        int member = 0;
        while (g->ctx[member] != c) ++member;
        const int cnt = (int) idx.size();
        std::vector<int64_t> o2(cnt + 1, 0);
        for (int k = 0; k < cnt; ++k) o2[k + 1] = o2[k] + (offs[idx[k] + 1] - offs[idx[k]]);
        std::vector<uint8_t> cd((size_t) o2[cnt]);
        std::vector<int32_t> l(cnt), r(cnt), st(cnt), rec((size_t) cnt * out_cap);
        for (int k = 0; k < cnt; ++k) {
            memcpy(cd.data() + o2[k], codes + offs[idx[k]], (size_t) (o2[k + 1] - o2[k]));
            l[k] = left[idx[k]]; r[k] = right[idx[k]]; st[k] = stop_at ? stop_at[idx[k]] : 0;
        }
        const int rc = spdp_blk_vote(c, ix[member], cd.data(), o2.data(), l.data(), r.data(), stop_at ? st.data() : nullptr, cnt,
                                     rec.data(), out_cap, nullptr);
        if (rc == 0)
            for (int k = 0; k < cnt; ++k) memcpy(out + (size_t) idx[k] * out_cap, rec.data() + (size_t) k * out_cap, (size_t) out_cap * 4);
        return rc;
    });
}

// map + align with the queries sharded over the members by length.  call(ctx, member, codes, offs, cnt, ...) runs one member's
// shard: its queries' codes gathered in caller order, renumbered 0 .. cnt - 1
extern "C++" {
namespace {
struct Shard {                          // a member's queries, gathered
    std::vector<int64_t> offs;
    std::vector<uint8_t> codes;
    Shard(const std::vector<int>& idx, const uint8_t* codes_, const int64_t* offs_) : offs(idx.size() + 1, 0)
    {
        const size_t cnt = idx.size();
        for (size_t k = 0; k < cnt; ++k) offs[k + 1] = offs[k] + (offs_[idx[k] + 1] - offs_[idx[k]]);
        codes.resize((size_t) offs[cnt]);
        for (size_t k = 0; k < cnt; ++k) memcpy(codes.data() + offs[k], codes_ + offs_[idx[k]], (size_t) (offs[k + 1] - offs[k]));
    }
};
int member_of(const SpdpGroup* g, const SpdpContext* c)
{
    int member = 0;
    while (g->ctx[member] != c) ++member;
    return member;
}
std::vector<int64_t> query_costs(const int64_t* offs, int n)
{
    std::vector<int64_t> cost(std::max(n, 0));
    for (int i = 0; i < n; ++i) cost[i] = 1 + offs[i + 1] - offs[i];
    return cost;
}

// one gene per query (spdp_map_align_s / _h): genes[n] of the caller; *exons malloc'ed, a member's exons in one run
template <typename CALL>
int group_map_best(SpdpGroup* g, const char* who, const uint8_t* codes, const int64_t* offs, int32_t n,
                   SpdpMapGene* genes, SpdpMapExon** exons, CALL&& call)
{
    const int w = g ? (int) g->ctx.size() : 0;
    std::vector<std::vector<SpdpMapExon>> part(std::max(w, 1));        // a member's exons, its genes' exon_off relative to them
    std::vector<std::vector<int>> whose(std::max(w, 1));
    const int rc = fan_out_idx(g, n, query_costs(offs, n), [&](SpdpContext* c, const std::vector<int>& idx) {
        const int member = member_of(g, c);
        const int cnt = (int) idx.size();
        Shard sh(idx, codes, offs);
        std::vector<SpdpMapGene> gn(cnt);
        SpdpMapExon* ex = nullptr;
        const int r = call(c, member, sh.codes.data(), sh.offs.data(), cnt, gn.data(), &ex);
        if (r >= 0) {
            size_t ne = 0;
            for (int k = 0; k < cnt; ++k) { genes[idx[k]] = gn[k]; ne = std::max<size_t>(ne, (size_t) gn[k].exon_off + gn[k].n_exons); }
            if (ex) part[member].assign(ex, ex + ne);
            whose[member] = idx;
        }
        free(ex);
        return r;
    });
    if (rc < 0) return rc;
    size_t total = 0;
    for (int r = 0; r < w; ++r) total += part[r].size();
    *exons = (SpdpMapExon*) malloc(sizeof(SpdpMapExon) * std::max<size_t>(total, 1));
    if (!*exons) { g->err = std::string(who) + ": out of memory"; return -1; }
    size_t base = 0;
    for (int r = 0; r < w; ++r) {
        if (!part[r].empty()) memcpy(*exons + base, part[r].data(), sizeof(SpdpMapExon) * part[r].size());
        for (int i : whose[r]) genes[i].exon_off += (int64_t) base;
        base += part[r].size();
    }
    return rc;
}

// lists of genes per query (the _multi entries): gene_off[n + 1] of the caller, *genes and *exons malloc'ed, both in the
// caller's query order
template <typename CALL>
int group_map_multi(SpdpGroup* g, const char* who, const uint8_t* codes, const int64_t* offs, int32_t n,
                    int64_t* gene_off, SpdpMapGene** genes, SpdpMapExon** exons, CALL&& call)
{
    const int w = g ? (int) g->ctx.size() : 0;
    struct Part { std::vector<int64_t> off; std::vector<SpdpMapGene> gn; std::vector<SpdpMapExon> ex; };
    std::vector<Part> part(std::max(w, 1));
    std::vector<std::pair<int, int>> at(std::max(n, 0), {-1, 0});     // query -> (member, its number there)
    const int rc = fan_out_idx(g, n, query_costs(offs, n), [&](SpdpContext* c, const std::vector<int>& idx) {
        const int member = member_of(g, c);
        const int cnt = (int) idx.size();
        Shard sh(idx, codes, offs);
        Part& P = part[member];
        P.off.assign(cnt + 1, 0);
        SpdpMapGene* gn = nullptr;
        SpdpMapExon* ex = nullptr;
        const int r = call(c, member, sh.codes.data(), sh.offs.data(), cnt, P.off.data(), &gn, &ex);
        if (r >= 0) {
            size_t ne = 0;
            for (int64_t j = 0; j < P.off[cnt]; ++j) ne = std::max<size_t>(ne, (size_t) gn[j].exon_off + gn[j].n_exons);
            P.gn.assign(gn, gn + P.off[cnt]);
            P.ex.assign(ex, ex + ne);
            for (int k = 0; k < cnt; ++k) at[idx[k]] = {member, k};
        }
        free(gn); free(ex);
        return r;
    });
    if (rc < 0) return rc;
    size_t ng = 0, ne = 0;
    for (int r = 0; r < w; ++r) { ng += part[r].gn.size(); ne += part[r].ex.size(); }
    *genes = (SpdpMapGene*) malloc(sizeof(SpdpMapGene) * std::max<size_t>(ng, 1));
    *exons = (SpdpMapExon*) malloc(sizeof(SpdpMapExon) * std::max<size_t>(ne, 1));
    if (!*genes || !*exons) {
        free(*genes); *genes = nullptr; free(*exons); *exons = nullptr;
        g->err = std::string(who) + ": out of memory"; return -1;
    }
    int64_t k = 0, o = 0;
    gene_off[0] = 0;
    for (int i = 0; i < n; ++i) {
        if (at[i].first >= 0) {
            const Part& P = part[at[i].first];
            for (int64_t j = P.off[at[i].second]; j < P.off[at[i].second + 1]; ++j, ++k) {
                SpdpMapGene G = P.gn[j];
                if (G.n_exons > 0) memcpy(*exons + o, P.ex.data() + G.exon_off, sizeof(SpdpMapExon) * G.n_exons);
                G.exon_off = o;
                o += G.n_exons;
                (*genes)[k] = G;
            }
        }
        gene_off[i + 1] = k;
    }
    return rc;
}
}   // namespace
}   // extern "C++"

int spdp_group_map_align_s(SpdpGroup* g, const SpdpBlkIndex* const* ix, const SpdpBlkIndexDesc* hix, const SpdpGenome* genome,
                           const SpdpScoring* sc, const SpdpSeedParams* sp, const SpdpSignalModel* sigmodel,
                           const SpdpBlkFindParams* fprm, const SpdpRescoreParams* rp,
                           const uint8_t* codes, const int64_t* offs, int32_t n, int32_t ori,
                           SpdpMapGene* genes, SpdpMapExon** exons)
{
    if (!ix || !codes || !offs || !genes || !exons) { if (g) g->err = "spdp_group_map_align_s: null argument"; return -1; }
    *exons = nullptr;
    return group_map_best(g, "spdp_group_map_align_s", codes, offs, n, genes, exons,
                          [&](SpdpContext* c, int member, const uint8_t* cd, const int64_t* o2, int cnt, SpdpMapGene* gn, SpdpMapExon** ex) {
        return spdp_map_align_s(c, ix[member], hix, genome, sc, sp, sigmodel, fprm, rp, cd, o2, cnt, ori, gn, ex, nullptr);
    });
}

int spdp_group_map_align_h(SpdpGroup* g, const SpdpBlkIndex* const* ix, const SpdpBlkIndexDesc* hix, const SpdpGenome* genome,
                           const SpdpScoringH* sc, const SpdpSeedParams* sp, const SpdpSignalModelH* sigmodel,
                           const SpdpBlkFindParams* fprm, const SpdpRescoreParamsH* rp,
                           const uint8_t* codes, const int64_t* offs, int32_t n,
                           SpdpMapGene* genes, SpdpMapExon** exons)
{
    if (!ix || !codes || !offs || !genes || !exons) { if (g) g->err = "spdp_group_map_align_h: null argument"; return -1; }
    *exons = nullptr;
    return group_map_best(g, "spdp_group_map_align_h", codes, offs, n, genes, exons,
                          [&](SpdpContext* c, int member, const uint8_t* cd, const int64_t* o2, int cnt, SpdpMapGene* gn, SpdpMapExon** ex) {
        return spdp_map_align_h(c, ix[member], hix, genome, sc, sp, sigmodel, fprm, rp, cd, o2, cnt, gn, ex, nullptr);
    });
}

int spdp_group_map_align_s_multi(SpdpGroup* g, const SpdpBlkIndex* const* ix, const SpdpBlkIndexDesc* hix, const SpdpGenome* genome,
                                 const SpdpScoring* sc, const SpdpSeedParams* sp, const SpdpSignalModel* sigmodel,
                                 const SpdpBlkFindParams* fprm, const SpdpRescoreParams* rp,
                                 const uint8_t* codes, const int64_t* offs, int32_t n, int32_t ori, int32_t all_out,
                                 int64_t* gene_off, SpdpMapGene** genes, SpdpMapExon** exons)
{
    if (!ix || !codes || !offs || !gene_off || !genes || !exons) { if (g) g->err = "spdp_group_map_align_s_multi: null argument"; return -1; }
    *genes = nullptr; *exons = nullptr;
    return group_map_multi(g, "spdp_group_map_align_s_multi", codes, offs, n, gene_off, genes, exons,
                           [&](SpdpContext* c, int member, const uint8_t* cd, const int64_t* o2, int cnt, int64_t* go, SpdpMapGene** gn, SpdpMapExon** ex) {
        return spdp_map_align_s_multi(c, ix[member], hix, genome, sc, sp, sigmodel, fprm, rp, cd, o2, cnt, ori, all_out, go, gn, ex, nullptr);
    });
}

int spdp_group_map_align_h_multi(SpdpGroup* g, const SpdpBlkIndex* const* ix, const SpdpBlkIndexDesc* hix, const SpdpGenome* genome,
                                 const SpdpScoringH* sc, const SpdpSeedParams* sp, const SpdpSignalModelH* sigmodel,
                                 const SpdpBlkFindParams* fprm, const SpdpRescoreParamsH* rp,
                                 const uint8_t* codes, const int64_t* offs, int32_t n, int32_t all_out,
                                 int64_t* gene_off, SpdpMapGene** genes, SpdpMapExon** exons)
{
    if (!ix || !codes || !offs || !gene_off || !genes || !exons) { if (g) g->err = "spdp_group_map_align_h_multi: null argument"; return -1; }
    *genes = nullptr; *exons = nullptr;
    return group_map_multi(g, "spdp_group_map_align_h_multi", codes, offs, n, gene_off, genes, exons,
                           [&](SpdpContext* c, int member, const uint8_t* cd, const int64_t* o2, int cnt, int64_t* go, SpdpMapGene** gn, SpdpMapExon** ex) {
        return spdp_map_align_h_multi(c, ix[member], hix, genome, sc, sp, sigmodel, fprm, rp, cd, o2, cnt, all_out, go, gn, ex, nullptr);
    });
}

// ---- the unspliced aligner, the protein-database search, the locus search and the _prep / _dispersed map + align entries ----------
// The same rule: the queries sharded by cost, every member the single-context entry on its shard from its own thread, nothing
// exchanged.  What comes back ragged -- pooled lists, side arrays behind offset fields, records that name their query -- is put
// into the caller's order by spdp_group_gather.h.  n <= 0 is handed to the first member as it is, so that a group answers an
// empty call (and refuses a bad one) exactly as a context does.
extern "C++" {
namespace {
using spdp_gather::Part;
using spdp_gather::Place;

double wall_since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); }

// member r runs call(r, ctx, its query numbers in caller order); idx: who got what.  A member's -1 ends the call with its message.
template <typename F>
int fan_out_members(SpdpGroup* g, int n, const std::vector<int64_t>& cost, std::vector<std::vector<int>>& idx, std::vector<int>& rc, F&& call)
{
    const int w = (int) g->ctx.size();
    idx = balanced(cost, w);
    g->shard_of.assign((size_t) std::max(n, 0), 0);
    rc.assign(w, 0);
    std::vector<std::thread> th;
    for (int r = 0; r < w; ++r) {
        if (idx[r].empty()) continue;
        for (int i : idx[r]) g->shard_of[i] = r;
        th.emplace_back([&, r]() {
            (void) hipSetDevice(g->ctx[r]->device);
            try { rc[r] = call(r, g->ctx[r], idx[r]); } catch (...) { rc[r] = -2; }
        });
    }
    for (std::thread& t : th) t.join();
    int worst = 0;
    for (int r = 0; r < w; ++r) {
        if (rc[r] < 0) {
            g->err = "device " + std::to_string(g->ctx[r]->device) + ": " + (rc[r] == -2 ? std::string("out of host memory") : g->ctx[r]->err);
            return -1;
        }
        worst |= rc[r];
    }
    return worst;
}

// an empty (or negative) call: the first member's answer is the group's
int first_member_says(SpdpGroup* g, int rc)
{
    g->shard_of.clear();
    if (rc < 0) g->err = "device " + std::to_string(g->ctx[0]->device) + ": " + g->ctx[0]->err;
    return rc;
}

bool no_group(SpdpGroup* g, const void* ix, const char* who)
{
    if (!g || g->ctx.empty()) return true;
    if (!ix) { g->err = std::string(who) + ": null argument"; return true; }
    return false;
}

// a phase lasts as long as its slowest member
struct PhaseSeconds {
    std::vector<double> of;
    int k;
    PhaseSeconds(int w, int k_) : of((size_t) w * k_, 0.0), k(k_) {}
    double* member(int r) { return of.data() + (size_t) r * k; }
    void max_into(double* seconds) const
    {
        if (!seconds) return;
        for (int j = 0; j < k; ++j) { seconds[j] = 0.0; for (size_t r = 0; r * k < of.size(); ++r) seconds[j] = std::max(seconds[j], of[r * k + j]); }
    }
};

std::vector<int64_t> costs_b(const SpdpScoring* sc, const SpdpProblem* probs, int n)
{
    std::vector<int64_t> c((size_t) std::max(n, 0), 1);
    if (!sc || !probs) return c;                        // (the members refuse the null argument)
    for (int i = 0; i < n; ++i) { SpdpWindow w; spdp_stripe(&probs[i], sc->sh, &w); c[i] = spdp_cells_b(&probs[i], &w); }
    return c;
}

// alignments of the unspliced aligner: out[i] of the caller; call(ctx, idx, the member's problems, cnt, its alignments).  Nothing is
// handed out unless every member answered: the alignments of those that did are released, out[i].skl = NULL.
template <typename CALL>
int group_align_b(SpdpGroup* g, const SpdpScoring* sc, const SpdpProblem* probs, int n, SpdpAlignment* out, CALL&& call)
{
    const int w = (int) g->ctx.size();
    std::vector<std::vector<int>> idx;
    std::vector<int> rcs;
    std::vector<std::vector<SpdpAlignment>> mine((size_t) w);
    const int rc = fan_out_members(g, n, costs_b(sc, probs, n), idx, rcs, [&](int r, SpdpContext* c, const std::vector<int>& ix) {
        const std::vector<SpdpProblem> p = spdp_gather::pick(ix, probs);
        mine[r] = spdp_gather::pick(ix, (const SpdpAlignment*) out);
        return call(c, ix, p.empty() ? nullptr : p.data(), (int) ix.size(), mine[r].empty() ? nullptr : mine[r].data());
    });
    if (rc < 0) {
        for (int r = 0; r < w; ++r) if (rcs[r] >= 0 && !mine[r].empty()) spdp_free_alignments(mine[r].data(), (int) mine[r].size());
        for (int i = 0; out && i < n; ++i) { out[i].score = SPDP_NEVSEL; out[i].n_skl = 0; out[i].skl = nullptr; }
        return -1;
    }
    for (int r = 0; r < w; ++r) spdp_gather::scatter(idx[r], mine[r].data(), out);
    return rc;
}

// the genes of a map + align entry: per query a list (gene_off != NULL: *genes malloc'ed) or exactly one record (gene_off == NULL:
// genes_fixed[n] of the caller), *exons and, for the dispersed entries, *part malloc'ed.  call(member, ctx, idx, codes, offs, cnt,
// gene_off, genes, exons, part, seconds) runs one member's shard and scatters what it has per query (covered, tails) itself.
template <typename CALL>
int group_genes(SpdpGroup* g, const char* who, const uint8_t* codes, const int64_t* offs, int32_t n, int64_t* gene_off, SpdpMapGene* genes_fixed,
                SpdpMapGene** genes, SpdpMapExon** exons, int32_t** part, double* seconds, CALL&& call)
{
    const int w = (int) g->ctx.size();
    std::vector<Part<SpdpMapGene, SpdpMapExon>> got((size_t) w);
    std::vector<Part<int32_t>> which((size_t) w);
    PhaseSeconds sec(w, 4);
    std::vector<std::vector<int>> idx;
    std::vector<int> rcs;
    const auto exon_count = [](const SpdpMapGene& G) { return G.n_exons; };
    const int rc = fan_out_members(g, n, query_costs(offs, n), idx, rcs, [&](int r, SpdpContext* c, const std::vector<int>& ix) {
        const int cnt = (int) ix.size();
        Shard sh(ix, codes, offs);
        Part<SpdpMapGene, SpdpMapExon>& P = got[r];
        P.off.assign((size_t) cnt + 1, 0);
        std::vector<SpdpMapGene> fixed((size_t) (gene_off ? 0 : cnt));
        SpdpMapGene* gn = nullptr;
        SpdpMapExon* ex = nullptr;
        int32_t* pt = nullptr;
        const int rr = call(r, c, ix, sh.codes.data(), sh.offs.data(), cnt, gene_off ? P.off.data() : nullptr, gene_off ? nullptr : fixed.data(),
                            &gn, &ex, part ? &pt : nullptr, sec.member(r));
        if (rr >= 0) {
            if (gene_off) P.rec.assign(gn, gn + P.off[cnt]);
            else { P.rec = fixed; for (int k = 0; k <= cnt; ++k) P.off[k] = k; }
            const size_t ne = spdp_gather::side_extent(P.rec.data(), (int64_t) P.rec.size(), &SpdpMapGene::exon_off, exon_count);
            if (ne) P.side.assign(ex, ex + ne);
            if (part) { which[r].off = P.off; if (pt) which[r].rec.assign(pt, pt + P.off[cnt]); else which[r].rec.assign((size_t) P.off[cnt], 0); }
        }
        free(gn); free(ex); free(pt);
        return rr;
    });
    if (rc < 0) return rc;
    const std::vector<Place> at = spdp_gather::places(n, idx);
    const spdp_gather::Totals t = spdp_gather::totals(at, got, exon_count);
    SpdpMapGene* G = genes_fixed;
    if (gene_off) { *genes = (SpdpMapGene*) malloc(sizeof(SpdpMapGene) * std::max<size_t>(t.rec, 1)); G = *genes; }
    *exons = (SpdpMapExon*) malloc(sizeof(SpdpMapExon) * std::max<size_t>(t.side, 1));
    if (part) *part = (int32_t*) malloc(sizeof(int32_t) * std::max<size_t>(t.rec, 1));
    if (!G || !*exons || (part && !*part)) {
        if (gene_off) { free(*genes); *genes = nullptr; }
        free(*exons); *exons = nullptr;
        if (part) { free(*part); *part = nullptr; }
        g->err = std::string(who) + ": out of memory"; return -1;
    }
    spdp_gather::gather_lists(at, got, gene_off, G, *exons, &SpdpMapGene::exon_off, exon_count, [](SpdpMapGene&, int) {});
    if (part) spdp_gather::gather_lists(at, which, (int64_t*) nullptr, *part);
    sec.max_into(seconds);
    return rc;
}
}   // namespace
}   // extern "C++"

// ---- 1. the unspliced aligner: cost = spdp_cells_b on the window spdp_stripe gives; max_trace_bytes holds per member
int spdp_group_homscore_b(SpdpGroup* g, const SpdpScoring* sc, const SpdpUnsplicedParams* up, const SpdpProblem* probs, int n_probs, int32_t* scores)
{
    if (!g || g->ctx.empty()) return -1;
    if (n_probs <= 0) return first_member_says(g, spdp_homscore_b(g->ctx[0], sc, up, probs, n_probs, scores));
    std::vector<std::vector<int>> idx;
    std::vector<int> rcs;
    return fan_out_members(g, n_probs, costs_b(sc, probs, n_probs), idx, rcs, [&](int, SpdpContext* c, const std::vector<int>& ix) {
        const std::vector<SpdpProblem> p = spdp_gather::pick(ix, probs);
        std::vector<int32_t> s = spdp_gather::pick(ix, (const int32_t*) scores);
        const int rc = spdp_homscore_b(c, sc, up, p.empty() ? nullptr : p.data(), (int) ix.size(), s.empty() ? nullptr : s.data());
        if (rc >= 0) spdp_gather::scatter(ix, s.data(), scores);
        return rc;
    });
}

int spdp_group_align_b(SpdpGroup* g, const SpdpScoring* sc, const SpdpUnsplicedParams* up, const SpdpProblem* probs, int n_probs, SpdpAlignment* out)
{
    if (!g || g->ctx.empty()) return -1;
    if (n_probs <= 0) return first_member_says(g, spdp_align_b(g->ctx[0], sc, up, probs, n_probs, out));
    return group_align_b(g, sc, probs, n_probs, out, [&](SpdpContext* c, const std::vector<int>&, const SpdpProblem* p, int cnt, SpdpAlignment* o) {
        return spdp_align_b(c, sc, up, p, cnt, o);
    });
}

int spdp_group_align_b_seeded(SpdpGroup* g, const SpdpScoring* sc, const SpdpUnsplicedParams* up, const SpdpSeedParams* sp,
                              const SpdpProblem* probs, int n_probs, const SpdpJuxt* const* hsps, const int32_t* n_hsps,
                              const int32_t* lowest_level, const SpdpHspSource* src, SpdpAlignment* out)
{
    if (!g || g->ctx.empty()) return -1;
    if (n_probs <= 0) return first_member_says(g, spdp_align_b_seeded(g->ctx[0], sc, up, sp, probs, n_probs, hsps, n_hsps, lowest_level, src, out));
    // the refusal is the whole call's, asked once: a member whose pairs all bring HSPs would serve a bundle the call as a whole may not
    bool all_bring = hsps && n_hsps;
    for (int i = 0; all_bring && i < n_probs; ++i) all_bring = hsps[i] && n_hsps[i] > 0;
    if (const char* why = spdp_align_b_seeded_refusal(sc, up, sp, all_bring, src && src->units)) { g->err = std::string("spdp_align_b_seeded: ") + why; return -1; }
    return group_align_b(g, sc, probs, n_probs, out, [&](SpdpContext* c, const std::vector<int>& ix, const SpdpProblem* p, int cnt, SpdpAlignment* o) {
        const std::vector<const SpdpJuxt*> h = spdp_gather::pick(ix, hsps);
        const std::vector<int32_t> nh = spdp_gather::pick(ix, n_hsps), ll = spdp_gather::pick(ix, lowest_level);
        RemapSource rs = {src, ix.data()};
        SpdpHspSource local = {&rs, remap_units, remap_release};
        return spdp_align_b_seeded(c, sc, up, sp, p, cnt, hsps ? h.data() : nullptr, n_hsps ? nh.data() : nullptr, lowest_level ? ll.data() : nullptr,
                                   src ? &local : nullptr, o);
    });
}

// ---- 2. the protein-database search: cost = 1 + query length; one index per member
int spdp_group_blk_finds(SpdpGroup* g, const SpdpBlkIndex* const* ix, const SpdpBlkIndexDesc* hix, const SpdpBlkFindsParams* prm,
                         const uint8_t* codes, const int64_t* offs, const int32_t* left, const int32_t* right, int32_t n,
                         int32_t* out, int32_t out_cap, float* kernel_ms)
{
    if (no_group(g, ix, "spdp_group_blk_finds")) return -1;
    if (n <= 0) return first_member_says(g, spdp_blk_finds(g->ctx[0], ix[0], hix, prm, codes, offs, left, right, n, out, out_cap, kernel_ms));
    if (!codes || !offs || !left || !right || !out) { g->err = "spdp_blk_finds: null argument"; return -1; }
    std::vector<std::vector<int>> idx;
    std::vector<int> rcs;
    std::vector<float> ms(g->ctx.size(), 0.f);
    const int rc = fan_out_members(g, n, query_costs(offs, n), idx, rcs, [&](int r, SpdpContext* c, const std::vector<int>& mine) {
        const int cnt = (int) mine.size();
        Shard sh(mine, codes, offs);
        const std::vector<int32_t> l = spdp_gather::pick(mine, left), rt = spdp_gather::pick(mine, right);
        std::vector<int32_t> rec((size_t) cnt * (size_t) std::max(out_cap, 0), 0);
        const int rr = spdp_blk_finds(c, ix[r], hix, prm, sh.codes.data(), sh.offs.data(), l.data(), rt.data(), cnt, rec.data(), out_cap, &ms[r]);
        if (rr >= 0) spdp_gather::scatter(mine, rec.data(), out, (size_t) out_cap);
        return rr;
    });
    if (rc >= 0 && kernel_ms) *kernel_ms = *std::max_element(ms.begin(), ms.end());
    return rc;
}

int spdp_group_map_align_b(SpdpGroup* g, const SpdpBlkIndex* const* ix, const SpdpBlkIndexDesc* hix, const SpdpGenome* db,
                           const SpdpScoring* sc, const SpdpUnsplicedParams* up, const SpdpSeedParams* sp, const SpdpBlkFindsParams* fprm,
                           const uint8_t* codes, const int64_t* offs, int32_t n, int32_t all_out,
                           int64_t* hit_off, SpdpMapHitB** hits, SpdpSkl** corners, double* seconds)
{
    if (no_group(g, ix, "spdp_group_map_align_b")) return -1;
    if (n <= 0) return first_member_says(g, spdp_map_align_b(g->ctx[0], ix[0], hix, db, sc, up, sp, fprm, codes, offs, n, all_out, hit_off, hits, corners, seconds));
    if (!codes || !offs || !hit_off || !hits || !corners) { g->err = "spdp_map_align_b: null argument"; return -1; }
    *hits = nullptr; *corners = nullptr;
    const auto t_call = std::chrono::steady_clock::now();
    const int w = (int) g->ctx.size();
    std::vector<Part<SpdpMapHitB, SpdpSkl>> got((size_t) w);
    PhaseSeconds sec(w, 4);
    std::vector<std::vector<int>> idx;
    std::vector<int> rcs;
    const auto corner_count = [](const SpdpMapHitB& h) { return h.n_corners; };
    const int rc = fan_out_members(g, n, query_costs(offs, n), idx, rcs, [&](int r, SpdpContext* c, const std::vector<int>& mine) {
        const int cnt = (int) mine.size();
        Shard sh(mine, codes, offs);
        Part<SpdpMapHitB, SpdpSkl>& P = got[r];
        P.off.assign((size_t) cnt + 1, 0);
        SpdpMapHitB* h = nullptr;
        SpdpSkl* cn = nullptr;
        const int rr = spdp_map_align_b(c, ix[r], hix, db, sc, up, sp, fprm, sh.codes.data(), sh.offs.data(), cnt, all_out, P.off.data(), &h, &cn, sec.member(r));
        if (rr >= 0 && h) {
            P.rec.assign(h, h + P.off[cnt]);
            const size_t ne = spdp_gather::side_extent(h, P.off[cnt], &SpdpMapHitB::corner_off, corner_count);
            if (ne && cn) P.side.assign(cn, cn + ne);
        }
        free(h); free(cn);
        return rr;
    });
    if (rc < 0) return rc;
    const std::vector<Place> at = spdp_gather::places(n, idx);
    const spdp_gather::Totals t = spdp_gather::totals(at, got, corner_count);
    *hits = (SpdpMapHitB*) malloc(sizeof(SpdpMapHitB) * std::max<size_t>(t.rec, 1));
    *corners = (SpdpSkl*) malloc(sizeof(SpdpSkl) * std::max<size_t>(t.side, 1));
    if (!*hits || !*corners) { free(*hits); free(*corners); *hits = nullptr; *corners = nullptr; g->err = "spdp_group_map_align_b: out of memory"; return -1; }
    spdp_gather::gather_lists(at, got, hit_off, *hits, *corners, &SpdpMapHitB::corner_off, corner_count, [](SpdpMapHitB&, int) {});
    sec.max_into(seconds);
    if (seconds) seconds[3] = wall_since(t_call);       // "the call" is the group's
    return rc;
}

// ---- 3. the locus search: loci query by query in the caller's order, SpdpLocus.query in the caller's numbers
int spdp_group_blk_find(SpdpGroup* g, const SpdpBlkIndex* const* ix, const SpdpBlkIndexDesc* hix, const SpdpGenome* genome,
                        const struct SpdpWilipModel* model, const SpdpScoring* sc, const SpdpBlkFindParams* prm,
                        const uint8_t* codes, const int64_t* offs, const int32_t* left, const int32_t* right, int32_t n,
                        SpdpLocus** loci, int32_t* n_loci, SpdpJuxt** hsps, int32_t* status)
{
    if (no_group(g, ix, "spdp_group_blk_find")) return -1;
    if (n <= 0) return first_member_says(g, spdp_blk_find(g->ctx[0], ix[0], hix, genome, model, sc, prm, codes, offs, left, right, n, loci, n_loci, hsps, status));
    if (!codes || !offs || !left || !right || !loci || !n_loci || !hsps) { g->err = "spdp_blk_find: null argument"; return -1; }
    *loci = nullptr; *hsps = nullptr; *n_loci = 0;
    const int w = (int) g->ctx.size();
    std::vector<Part<SpdpLocus, SpdpJuxt>> got((size_t) w);
    std::vector<std::vector<int>> idx;
    std::vector<int> rcs;
    const auto hsp_count = [](const SpdpLocus& L) { return L.n_hsp + 1; };      // (the closing slot behind the last HSP)
    const int rc = fan_out_members(g, n, query_costs(offs, n), idx, rcs, [&](int r, SpdpContext* c, const std::vector<int>& mine) {
        const int cnt = (int) mine.size();
        Shard sh(mine, codes, offs);
        const std::vector<int32_t> l = spdp_gather::pick(mine, left), rt = spdp_gather::pick(mine, right);
        std::vector<int32_t> st = spdp_gather::pick(mine, (const int32_t*) status);
        SpdpLocus* lc = nullptr;
        SpdpJuxt* hs = nullptr;
        int32_t nl = 0;
        const int rr = spdp_blk_find(c, ix[r], hix, genome, model, sc, prm, sh.codes.data(), sh.offs.data(), l.data(), rt.data(), cnt, &lc, &nl, &hs,
                                     status ? st.data() : nullptr);
        if (rr >= 0) {
            Part<SpdpLocus, SpdpJuxt>& P = got[r];
            P.off = spdp_gather::offsets_by_query(lc, (int64_t) nl, cnt, &SpdpLocus::query);
            if (lc) P.rec.assign(lc, lc + nl);
            const size_t ne = spdp_gather::side_extent(lc, (int64_t) nl, &SpdpLocus::hsp_off, hsp_count);
            if (ne && hs) P.side.assign(hs, hs + ne);
            spdp_gather::scatter(mine, st.data(), status);
        }
        free(lc); free(hs);
        return rr;
    });
    if (rc < 0) return rc;
    const std::vector<Place> at = spdp_gather::places(n, idx);
    const spdp_gather::Totals t = spdp_gather::totals(at, got, hsp_count);
    *loci = (SpdpLocus*) malloc(sizeof(SpdpLocus) * std::max<size_t>(t.rec, 1));
    *hsps = (SpdpJuxt*) malloc(sizeof(SpdpJuxt) * std::max<size_t>(t.side, 1));
    if (!*loci || !*hsps) { free(*loci); free(*hsps); *loci = nullptr; *hsps = nullptr; g->err = "spdp_group_blk_find: out of memory"; return -1; }
    spdp_gather::gather_lists(at, got, (int64_t*) nullptr, *loci, *hsps, &SpdpLocus::hsp_off, hsp_count, [](SpdpLocus& L, int q) { L.query = q; });
    *n_loci = (int32_t) t.rec;
    return rc;
}

// ---- 4. the map + align entries with the preparation in front, and the dispersed ones
int spdp_group_map_align_s_prep(SpdpGroup* g, const SpdpBlkIndex* const* ix, const SpdpBlkIndexDesc* hix, const SpdpGenome* genome,
                                const SpdpScoring* sc, const SpdpSeedParams* sp, const SpdpSignalModel* sigmodel,
                                const SpdpBlkFindParams* fprm, const SpdpRescoreParams* rp,
                                const uint8_t* codes, const int64_t* offs, int32_t n, const SpdpQueryPrep* prep,
                                SpdpMapGene* genes, SpdpMapExon** exons, double* seconds, SpdpQueryTail* tails)
{
    if (no_group(g, ix, "spdp_group_map_align_s_prep")) return -1;
    if (n <= 0) return first_member_says(g, spdp_map_align_s_prep(g->ctx[0], ix[0], hix, genome, sc, sp, sigmodel, fprm, rp, codes, offs, n, prep, genes, exons, seconds, tails));
    if (!codes || !offs || !genes || !exons) { g->err = "spdp_map_align_s_prep: null argument"; return -1; }
    *exons = nullptr;
    return group_genes(g, "spdp_group_map_align_s_prep", codes, offs, n, nullptr, genes, nullptr, exons, nullptr, seconds,
                       [&](int r, SpdpContext* c, const std::vector<int>& mine, const uint8_t* cd, const int64_t* o2, int cnt, int64_t*, SpdpMapGene* gn,
                           SpdpMapGene**, SpdpMapExon** ex, int32_t**, double* sec) {
        std::vector<SpdpQueryTail> tl((size_t) cnt);
        const int rc = spdp_map_align_s_prep(c, ix[r], hix, genome, sc, sp, sigmodel, fprm, rp, cd, o2, cnt, prep, gn, ex, sec, tails ? tl.data() : nullptr);
        if (rc >= 0) spdp_gather::scatter(mine, tl.data(), tails);
        return rc;
    });
}

int spdp_group_map_align_s_multi_prep(SpdpGroup* g, const SpdpBlkIndex* const* ix, const SpdpBlkIndexDesc* hix, const SpdpGenome* genome,
                                      const SpdpScoring* sc, const SpdpSeedParams* sp, const SpdpSignalModel* sigmodel,
                                      const SpdpBlkFindParams* fprm, const SpdpRescoreParams* rp,
                                      const uint8_t* codes, const int64_t* offs, int32_t n, const SpdpQueryPrep* prep, int32_t all_out,
                                      int64_t* gene_off, SpdpMapGene** genes, SpdpMapExon** exons, double* seconds, SpdpQueryTail* tails)
{
    if (no_group(g, ix, "spdp_group_map_align_s_multi_prep")) return -1;
    if (n <= 0) return first_member_says(g, spdp_map_align_s_multi_prep(g->ctx[0], ix[0], hix, genome, sc, sp, sigmodel, fprm, rp, codes, offs, n, prep, all_out,
                                                                         gene_off, genes, exons, seconds, tails));
    if (!codes || !offs || !gene_off || !genes || !exons) { g->err = "spdp_map_align_s_multi_prep: null argument"; return -1; }
    *genes = nullptr; *exons = nullptr;
    return group_genes(g, "spdp_group_map_align_s_multi_prep", codes, offs, n, gene_off, nullptr, genes, exons, nullptr, seconds,
                       [&](int r, SpdpContext* c, const std::vector<int>& mine, const uint8_t* cd, const int64_t* o2, int cnt, int64_t* go, SpdpMapGene*,
                           SpdpMapGene** gn, SpdpMapExon** ex, int32_t**, double* sec) {
        std::vector<SpdpQueryTail> tl((size_t) cnt);
        const int rc = spdp_map_align_s_multi_prep(c, ix[r], hix, genome, sc, sp, sigmodel, fprm, rp, cd, o2, cnt, prep, all_out, go, gn, ex, sec,
                                                   tails ? tl.data() : nullptr);
        if (rc >= 0) spdp_gather::scatter(mine, tl.data(), tails);
        return rc;
    });
}

int spdp_group_map_align_s_dispersed(SpdpGroup* g, const SpdpBlkIndex* const* ix, const SpdpBlkIndexDesc* hix, const SpdpGenome* genome,
                                     const SpdpScoring* sc, const SpdpSeedParams* sp, const SpdpSignalModel* sigmodel,
                                     const SpdpBlkFindParams* fprm, const SpdpRescoreParams* rp,
                                     const uint8_t* codes, const int64_t* offs, int32_t n, int32_t ori, const SpdpQueryPrep* prep,
                                     int32_t min_seg_len, int64_t* gene_off, SpdpMapGene** genes, SpdpMapExon** exons, int32_t** part,
                                     int32_t* covered, double* seconds, SpdpQueryTail* tails)
{
    if (no_group(g, ix, "spdp_group_map_align_s_dispersed")) return -1;
    if (n <= 0) return first_member_says(g, spdp_map_align_s_dispersed(g->ctx[0], ix[0], hix, genome, sc, sp, sigmodel, fprm, rp, codes, offs, n, ori, prep, min_seg_len,
                                                                        gene_off, genes, exons, part, covered, seconds, tails));
    if (!codes || !offs || !gene_off || !genes || !exons || !part) { g->err = "spdp_map_align_s_dispersed: null argument"; return -1; }
    *genes = nullptr; *exons = nullptr; *part = nullptr;
    return group_genes(g, "spdp_group_map_align_s_dispersed", codes, offs, n, gene_off, nullptr, genes, exons, part, seconds,
                       [&](int r, SpdpContext* c, const std::vector<int>& mine, const uint8_t* cd, const int64_t* o2, int cnt, int64_t* go, SpdpMapGene*,
                           SpdpMapGene** gn, SpdpMapExon** ex, int32_t** pt, double* sec) {
        std::vector<SpdpQueryTail> tl((size_t) cnt);
        std::vector<int32_t> cov((size_t) 2 * cnt, 0);
        const int rc = spdp_map_align_s_dispersed(c, ix[r], hix, genome, sc, sp, sigmodel, fprm, rp, cd, o2, cnt, ori, prep, min_seg_len, go, gn, ex, pt,
                                                  covered ? cov.data() : nullptr, sec, tails ? tl.data() : nullptr);
        if (rc >= 0) { spdp_gather::scatter(mine, tl.data(), tails); spdp_gather::scatter(mine, cov.data(), covered, 2); }
        return rc;
    });
}

int spdp_group_map_align_h_dispersed(SpdpGroup* g, const SpdpBlkIndex* const* ix, const SpdpBlkIndexDesc* hix, const SpdpGenome* genome,
                                     const SpdpScoringH* sc, const SpdpSeedParams* sp, const SpdpSignalModelH* sigmodel,
                                     const SpdpBlkFindParams* fprm, const SpdpRescoreParamsH* rp,
                                     const uint8_t* codes, const int64_t* offs, int32_t n, int32_t min_seg_len,
                                     int64_t* gene_off, SpdpMapGene** genes, SpdpMapExon** exons, int32_t** part,
                                     int32_t* covered, double* seconds)
{
    if (no_group(g, ix, "spdp_group_map_align_h_dispersed")) return -1;
    if (n <= 0) return first_member_says(g, spdp_map_align_h_dispersed(g->ctx[0], ix[0], hix, genome, sc, sp, sigmodel, fprm, rp, codes, offs, n, min_seg_len,
                                                                        gene_off, genes, exons, part, covered, seconds));
    if (!codes || !offs || !gene_off || !genes || !exons || !part) { g->err = "spdp_map_align_h_dispersed: null argument"; return -1; }
    *genes = nullptr; *exons = nullptr; *part = nullptr;
    return group_genes(g, "spdp_group_map_align_h_dispersed", codes, offs, n, gene_off, nullptr, genes, exons, part, seconds,
                       [&](int r, SpdpContext* c, const std::vector<int>& mine, const uint8_t* cd, const int64_t* o2, int cnt, int64_t* go, SpdpMapGene*,
                           SpdpMapGene** gn, SpdpMapExon** ex, int32_t** pt, double* sec) {
        std::vector<int32_t> cov((size_t) 2 * cnt, 0);
        const int rc = spdp_map_align_h_dispersed(c, ix[r], hix, genome, sc, sp, sigmodel, fprm, rp, cd, o2, cnt, min_seg_len, go, gn, ex, pt,
                                                  covered ? cov.data() : nullptr, sec);
        if (rc >= 0) spdp_gather::scatter(mine, cov.data(), covered, 2);
        return rc;
    });
}

// which member ran problem i in the last group call (cost-balanced: spdp_cells per problem, longest first)
int spdp_group_last_shards(const SpdpGroup* g, int32_t* member, int n)
{
    if (!g || !member) return -1;
    for (int i = 0; i < n && i < (int) g->shard_of.size(); ++i) member[i] = g->shard_of[i];
    return (int) g->shard_of.size();
}

}   // extern "C"
