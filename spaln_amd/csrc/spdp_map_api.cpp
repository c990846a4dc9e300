// spdp_map_api.cpp -- map and align in one call (include/spdp.h "map and align"): block search -> regions + splice signals -> seeded
// alignment -> rescoring -> the loci that stay, for a batch of cDNA queries (spdp_map_align_s*) or of protein queries against the
// translated index (spdp_map_align_h*).  What the reference's per-query driver does around alignS_ng when the genome is searched
// (src/spaln.cc:880-1010: blkaln / spalign2, genomicseq at :913 reading the region and building its Exinon), batched: all loci of a
// chunk of queries share one signal launch, one seeded call and one rescoring call.  Host code only; the device work is that of the
// entries it calls.
//
// One chain, written once for both kinds of query, serves three outputs: the best locus of a query (spdp_map_align_s / _h), the
// list of loci spaln -M prints (_multi, blkaln's selection at src/spaln.cc:913-976) and the dispersed loci of spaln -pr
// (_dispersed).  The chain hands every candidate locus, aligned and rescored, to a sink in the block search's order; the
// selections are sinks.
#include "spdp_internal.h"
#include "spdp_h_internal.h"
#include "spdp_region.h"
#include "spdp_hostcpus.h"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <new>
#include <numeric>
#include <vector>

int spdh_signals_run(SpdpContext* ctx, const SpdpSignalModelH* m, const std::vector<SigJobH>& jobs, SignalArgsH args, int pack);   // spdp_signals_api.cpp
const char* spdp_prep_refused(const SpdpQueryPrep* prep);                                                                          // spdp_polya_api.cpp
int spdp_blk_find_tlen(SpdpContext* ctx, const SpdpBlkIndex* ix, const SpdpBlkIndexDesc* hix, const SpdpGenome* genome,              // spdp_blk_api.cpp
                       const SpdpWilipModel* model, const SpdpScoring* sc, const SpdpBlkFindParams* prm,
                       const uint8_t* codes, const int64_t* offs, const int32_t* left, const int32_t* right, const int32_t* tlen, int32_t n,
                       SpdpLocus** loci, int32_t* n_loci, SpdpJuxt** hsps, int32_t* status);

namespace {

struct DevMem {                      // scoped device allocation
    void* p = nullptr;
    ~DevMem() { if (p) (void) hipFree(p); }
    hipError_t get(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 16)); }
    template <class T> T* as() const { return (T*) p; }
};

double since(std::chrono::steady_clock::time_point t)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
}

// one candidate locus after the walk and rescoring: what blkaln's Gsinfo of that locus holds when its loop is done
struct LocusOut {
    bool aligned;                    // the walk gave a skeleton (Gsinfo::skl)
    SpdpMapGene g;                   // chr, rvs, q_rev, score (Gsinfo::scr), val (fstat.val; 0 -- vclear -- when not aligned)
    std::vector<SpdpMapExon> ex;     // its exons as -O4 prints them
    int32_t rleft = 0, rright = 0;   // first exon's rleft, last exon's rright: the query range it covers, as the block search counts it
};
// called once per locus, in the block search's order (query by query, a query's loci as findblock listed them)
using LocusSink = std::function<void(const SpdpLocus& L, LocusOut&& o)>;

SpdpMapGene no_gene()
{
    SpdpMapGene g;
    g.chr = -1; g.rvs = 0; g.q_rev = 0; g.score = SPDP_NEVSEL; g.val = 0; g.n_loci = 0; g.n_exons = 0; g.exon_off = 0;
    return g;
}

// per query: the genes it reports, in order -> gene_off[n + 1] of the caller, *genes and *exons malloc'ed
struct Reported {
    std::vector<std::vector<SpdpMapGene>> genes;
    std::vector<std::vector<std::vector<SpdpMapExon>>> ex;
    explicit Reported(int n) : genes(n), ex(n) {}
};
int hand_out(SpdpContext* ctx, const char* who, const Reported& r, int n, int64_t* gene_off, SpdpMapGene** genes, SpdpMapExon** exons)
{
    size_t ng = 0, ne = 0;
    for (int i = 0; i < n; ++i) { ng += r.genes[i].size(); for (const auto& e : r.ex[i]) ne += e.size(); }
    *exons = (SpdpMapExon*) malloc(sizeof(SpdpMapExon) * std::max<size_t>(ne, 1));
    *genes = (SpdpMapGene*) malloc(sizeof(SpdpMapGene) * std::max<size_t>(ng, 1));
    if (!*exons || !*genes) { ctx->err = std::string(who) + ": out of memory"; return -1; }      // (the entry's frame frees what there is)
    size_t o = 0, k = 0;
    gene_off[0] = 0;
    for (int i = 0; i < n; ++i) {
        for (size_t j = 0; j < r.genes[i].size(); ++j, ++k) {
            SpdpMapGene G = r.genes[i][j];
            const std::vector<SpdpMapExon>& e = r.ex[i][j];
            G.exon_off = (int64_t) o; G.n_exons = (int32_t) e.size();
            if (!e.empty()) memcpy(*exons + o, e.data(), sizeof(SpdpMapExon) * e.size());
            o += e.size();
            (*genes)[k] = G;
        }
        gene_off[i + 1] = (int64_t) k;
    }
    return 0;
}

// the best locus of a query: the highest fstat.val of the aligned ones, the first on ties; no threshold (spdp_map_align_s / _h)
struct BestSink {
    std::vector<SpdpMapGene> best;
    std::vector<std::vector<SpdpMapExon>> ex;
    explicit BestSink(int n) : best(n, no_gene()), ex(n) {}
    void operator()(const SpdpLocus& L, LocusOut&& o)
    {
        if (!o.aligned) return;
        SpdpMapGene& G = best[L.query];
        ++G.n_loci;
        if (G.chr >= 0 && G.val >= o.g.val) return;
        const int32_t nl = G.n_loci;
        G = o.g; G.n_loci = nl;
        ex[L.query] = std::move(o.ex);
    }
    int finish(SpdpContext* ctx, const char* who, int n, SpdpMapGene* genes, SpdpMapExon** exons)
    {
        size_t ne = 0;
        for (int i = 0; i < n; ++i) ne += ex[i].size();
        *exons = (SpdpMapExon*) malloc(sizeof(SpdpMapExon) * std::max<size_t>(ne, 1));
        if (!*exons) { ctx->err = std::string(who) + ": out of memory"; return -1; }
        size_t o = 0;
        for (int i = 0; i < n; ++i) {
            genes[i] = best[i];
            genes[i].exon_off = (int64_t) o; genes[i].n_exons = (int32_t) ex[i].size();
            if (!ex[i].empty()) memcpy(*exons + o, ex[i].data(), sizeof(SpdpMapExon) * ex[i].size());
            o += ex[i].size();
        }
        return 0;
    }
};

// what spaln -M N prints of a query (blkaln, src/spaln.cc:913-976): every locus is dropped (scr = NEVSEL, not counted in n_out)
// whose walk failed or -- unless all_out (-pw) -- whose score is <= Vthr; ALL loci, the dropped ones too, are insertion-sorted by
// fstat.val (descending, stable); the first min(n_out, MaxOut) positions of that order are printed, those without a skeleton
// skipped.  So a locus dropped by the threshold keeps its place in the order and is printed when it lands in one of those slots.
// (v: one query's loci in the block search's order -> the printed ones)
void select_printed(std::vector<LocusOut>& v, int max_out, int all_out, int vthr, std::vector<SpdpMapGene>& genes, std::vector<std::vector<SpdpMapExon>>& ex)
{
    const int np = (int) v.size();
    int n_out = 0, n_aligned = 0;
    for (const LocusOut& o : v) {
        n_aligned += o.aligned;
        n_out += o.aligned && (all_out || o.g.score > vthr);
    }
    std::vector<int> odr(np);
    std::iota(odr.begin(), odr.end(), 0);
    for (int k = 1; k < np; ++k) {                         // (the reference's insertion sort: ties keep their order)
        const int l = odr[k];
        int m = k;
        while (--m >= 0 && v[l].g.val > v[odr[m]].g.val) odr[m + 1] = odr[m];
        odr[m + 1] = l;
    }
    n_out = std::min(n_out, max_out);
    for (int k = 0; k < n_out; ++k) {
        LocusOut& o = v[odr[k]];
        if (!o.aligned) continue;
        if (!all_out && o.g.score <= vthr) o.g.score = SPDP_NEVSEL;     // (dropped, printed all the same: its scr is NEVSEL by then)
        o.g.n_loci = n_aligned;
        genes.push_back(o.g);
        ex.push_back(std::move(o.ex));
    }
}

struct MultiSink {
    std::vector<std::vector<LocusOut>> all;
    int max_out, all_out, vthr;
    MultiSink(int n, int max_out_, int all_out_, int vthr_) : all(n), max_out(max_out_), all_out(all_out_), vthr(vthr_) {}
    void operator()(const SpdpLocus& L, LocusOut&& o) { all[L.query].push_back(std::move(o)); }
    int finish(SpdpContext* ctx, const char* who, int n, int64_t* gene_off, SpdpMapGene** genes, SpdpMapExon** exons)
    {
        Reported r(n);
        for (int i = 0; i < n; ++i) select_printed(all[i], max_out, all_out, vthr, r.genes[i], r.ex[i]);
        return hand_out(ctx, who, r, n, gene_off, genes, exons);
    }
};

// the checks the multi entries add: MaxOut as blkaln reads it, and an index whose queues were sized for it (Ncand = MaxOut + 10,
// src/blksrc.cc:2220)
int check_multi(SpdpContext* ctx, const char* who, const SpdpBlkIndexDesc* hix, const SpdpBlkFindParams* fprm)
{
    if (!hix || !fprm) { ctx->err = std::string(who) + ": null argument"; return -1; }
    if (fprm->max_out < 1 || fprm->max_out2 < fprm->max_out) {
        ctx->err = std::string(who) + ": max_out must be >= 1 and max_out2 >= max_out (spaln -M N[.M])"; return -1;
    }
    if (hix->ncand != fprm->max_out + 10) {
        ctx->err = std::string(who) + ": the index was made for another MaxOut (its ncand " + std::to_string(hix->ncand) + " != max_out + 10 = " +
                   std::to_string(fprm->max_out + 10) + "; SpdpBlkSearchOpts.max_out sets it)";
        return -1;
    }
    return 0;
}

// ---- the chain: block search -> regions + signals -> seeded walks -> rescoring -> sink -------------------------------------------
// Written once for both kinds of query.  A kind (KindS: cDNA, KindH: protein against the translated index, `spaln -W -KP`) holds what
// differs: the types, the layout of a chunk's staging block, and one function per step of a chunk.  What blkaln / genomicseq /
// spalign2 do per query (src/spaln.cc:846-1010, 1137-1152), for a batch: all loci of a chunk share one signal launch, one seeded
// call and one rescoring call.

// what a call holds whatever its queries are
struct ChainBase {
    const char* who;                                    // the entry that was called: its name stands in front of every message
    SpdpContext* ctx; const SpdpBlkIndex* ix; const SpdpBlkIndexDesc* hix; const SpdpGenome* genome;
    const SpdpSeedParams* sp; const SpdpBlkFindParams* fprm;
    const uint8_t* codes; const int64_t* offs; int32_t n;      // (codes: the normalised queries once a preparation has run)
    double sec[4] = {0, 0, 0, 0};                       // find, regions + signals, align, rescore
    int partial = 0;
    std::vector<int32_t> ql, qr;                        // every query's range
    int refuse(const std::string& why) { ctx->err = std::string(who) + ": " + why; return -1; }
};

// One chunk of loci between the steps.  Its arrays lie in one pinned block H of the context (it stays for the next call) and one
// device block of the same layout, T positions per array; slot j < m is locus j as the block search gave it, slot m + k (cDNA,
// ori = 3) locus k's other strand, right behind it in the arrays.  It owns the alignments and the rescored exons.
template <class Problem>
struct Chunk {
    const SpdpLocus* loci; int m, ns;
    const int32_t* rng;                                 // (may be null) the query range of locus k: rng[2 k] .. rng[2 k + 1]
    std::vector<int64_t> at;                            // first position of slot j
    int64_t tot = 0, T = 0;
    uint8_t* H = nullptr;
    std::vector<Problem> probs;
    std::vector<const SpdpJuxt*> hl;
    std::vector<int32_t> hn, low, orient;               // orient[k]: the walk took locus k's other-strand slot
    std::vector<SpdpAlignment> aln;
    std::vector<SpdpRescored> res;
    Chunk(const SpdpLocus* l, int m_, int slots, const int32_t* r)
        : loci(l), m(m_), ns(slots * m_), rng(r), at(ns), probs(ns), hl(m), hn(m), low(m, 0), orient(m, 0), aln(m), res(m)
    {}                                                  // (the vectors' records are zeroed)
    ~Chunk() { spdp_free_rescored(res.data(), m); spdp_free_alignments(aln.data(), m); }
    Chunk(const Chunk&) = delete;
    bool other(int j) const { return j >= m; }
    const SpdpLocus& locus(int j) const { return loci[j < m ? j : j - m]; }
    int32_t left(int j) const { const SpdpLocus& L = locus(j); return j < m ? L.left : L.len - L.right; }
    int32_t right(int j) const { const SpdpLocus& L = locus(j); return j < m ? L.right : L.len - L.left; }
};

// chunks of loci, chunk i = [b[i], b[i + 1]): as few as `limit` positions each allow, of equal size (a call's time is a chain of
// request latencies, not device work: DESIGN.md 6g -- so the larger a chunk the better, and a short last chunk costs as much as a
// full one); a locus larger than that is a chunk of its own
std::vector<int> cut_chunks(const std::vector<int64_t>& positions, int64_t limit)
{
    const int n = (int) positions.size();
    const int64_t all = std::accumulate(positions.begin(), positions.end(), (int64_t) 0);
    const int64_t n_chunks = std::max<int64_t>(1, (all + limit - 1) / limit);
    const int64_t per_chunk = (all + n_chunks - 1) / n_chunks;
    std::vector<int> b(1, 0);
    int64_t tot = 0;
    for (int k = 0; k < n; ++k) {
        if (k > b.back() && tot + positions[k] > per_chunk + (1 << 17)) { b.push_back(k); tot = 0; }
        tot += positions[k];
    }
    if (n) b.push_back(n);
    return b;
}

// ---- cDNA queries: spdp_signals, spdp_align_s_seeded (_ori3 with both orientations), spdp_skl_rng_s
struct KindS : ChainBase {
    using Problem = SpdpProblem;
    using Job = SigJob;
    // staging block: codes | sig5 | sig3 (int16) | cano5 | cano3 | dinc; len + 1 positions per slot.  The default limit is 16 GiB of
    // pinned host memory and as much on the device (a C4-sized batch of 125 000 ESTs x 2 strands x ~50 kb of loci is what reaches it)
    static constexpr int host_bytes = 8, dev_bytes = 8, pad = 1;
    static constexpr size_t default_mpos = 2048;
    const SpdpScoring* sc; const SpdpSignalModel* sigmodel; const SpdpRescoreParams* rp; int32_t ori;
    const SpdpQueryPrep* prep; bool prepares; SpdpQueryTail* tails_out;      // the _prep entries (include/spdp.h "query preparation")
    std::vector<SpdpQueryTail> tail;                    // empty: no preparation, or none that scans (polya_thr <= 0)
    std::vector<uint8_t> normal;
    std::vector<int32_t> qt;                            // Seq::tlen per query
    bool tailed = false;
    std::vector<uint8_t> codes_rc;                      // comrev() of every normalised query (ori = 3)
    SpdpSignalModel sigm; SpdpSeedParams spx;           // the caller's with both_ori set: Exinon(seq, pwd, ori == 3), src/spaln.cc:1143, 1150
    KindS(const ChainBase& b, const SpdpScoring* sc_, const SpdpSignalModel* sm, const SpdpRescoreParams* rp_, int32_t ori_,
          const SpdpQueryPrep* prep_ = nullptr, bool prepares_ = false, SpdpQueryTail* tails = nullptr)
        : ChainBase(b), sc(sc_), sigmodel(sm), rp(rp_), ori(ori_), prep(prep_), prepares(prepares_), tails_out(tails) {}
    const int32_t* tlen() const { return tailed ? qt.data() : nullptr; }
    bool prep_turned(int q) const { return tailed && tail[q].pol == 2; }   // the preparation reverse-complemented query q
    int slots() const { return ori == 3 ? 2 : 1; }
    const SpdpScoring* chain_costs() { return sc; }

    int refused()
    {
        // the _prep entries: the orientation is the preparation's (rmpolyA returns q_mns for every query: 3 whatever it finds, 1 under
        // -S1 where no T head is looked for -- so a batch never mixes orientations)
        if (prepares) {
            if (const char* why = spdp_prep_refused(prep)) return refuse(why);
            ori = prep->q_mns;
        }
        if (ori != 1 && ori != 3) return refuse("ori must be 1 (the query as given) or 3 (both orientations)");
        if (!sp->wilip) return refuse("SpdpSeedParams.wilip missing (the HSP searches of this call are the library's own)");
        sigm = *sigmodel; spx = *sp;
        if (ori == 3) sigm.both_ori = spx.both_ori = 1;
        return 0;
    }
    // the preparation (PolyA::rmpolyA, spdp_polya.hip): tails found, antisense queries turned; from here on `codes` are the
    // normalised queries and every reader of a query's range or length takes them from its record.  Then their other strand
    int prepare()
    {
        if (prepares && prep->polya_thr > 0) {
            tail.resize(n); normal.resize((size_t) offs[n]);
            if (spdp_polya_scan(ctx, codes, offs, n, prep, tail.data(), normal.data(), nullptr)) return -1;
            codes = normal.data();
            qt.resize(n);
            for (int i = 0; i < n; ++i) { ql[i] = tail[i].left; qr[i] = tail[i].right; qt[i] = tail[i].tlen; }
            if (tails_out) memcpy(tails_out, tail.data(), sizeof(SpdpQueryTail) * (size_t) n);
        } else if (prepares && tails_out && spdp_polya_scan_host(codes, offs, n, prep, tails_out, nullptr)) return refuse("bad query offsets");
        tailed = !tail.empty();
        if (ori == 3) {
            codes_rc.resize((size_t) offs[n]);
            on_host_threads(n, [&](int q) {
                const int64_t a0 = offs[q], len = offs[q + 1] - offs[q];
                for (int64_t i = 0; i < len; ++i) codes_rc[a0 + i] = spdp_region::other_strand(codes[a0 + len - 1 - i]);
            });
        }
        return 0;
    }

    // x.sig5 .. x.dinc of a SignalArgs or a problem: the arrays of block B, from position `at` on
    template <class X> static void lay(X& x, uint8_t* B, int64_t T, int64_t at)
    {
        x.sig5 = (int16_t*) (B + T) + at; x.sig3 = (int16_t*) (B + 3 * T) + at;
        x.cano5 = B + 5 * T + at; x.cano3 = B + 6 * T + at; x.dinc = B + 7 * T + at;
    }
    void cut(Chunk<Problem>& c, int j)
    {
        const SpdpLocus& L = c.locus(j);
        spdp_region::materialize_into(genome->codes, genome->chr_off, L.chr, L.base, L.len, (L.rvs != 0) != c.other(j), false, c.H + c.at[j]);
    }
    int signals(Chunk<Problem>& c, const std::vector<Job>& jobs, uint8_t* D)
    {
        SignalArgs A;
        memset(&A, 0, sizeof A);
        A.codes = D;
        lay(A, D, c.T, 0);
        return spdp_signals_run(ctx, &sigm, jobs, A, nullptr, nullptr);
    }
    void point(Chunk<Problem>& c, int j, Problem& P)
    {
        if (c.other(j)) P.a = codes_rc.data() + offs[c.locus(j).query];
        lay(P, c.H, c.T, c.at[j]);
    }
    int walk(Chunk<Problem>& c)
    {
        const int m = c.m;
        // Seq::tlen of every problem for the walks' own HSP searches; the reverse leg keeps the forward one's (alignS_ng turns the
        // query in place, which leaves tlen alone: there the bound cuts the transcript's end, the tail sits at the front)
        std::vector<int32_t> ptl;
        if (tailed) { ptl.resize(c.ns); for (int j = 0; j < c.ns; ++j) ptl[j] = tail[c.locus(j).query].tlen; }
        struct TlenSet { SpdpContext* c; ~TlenSet() { c->seed_a_tlen = nullptr; } } tlen_set{ctx};
        ctx->seed_a_tlen = tailed ? ptl.data() : nullptr;
        const int rc = ori == 3 ? spdp_align_s_seeded_ori3(ctx, sc, &spx, c.probs.data(), c.probs.data() + m, m, c.hl.data(), c.hn.data(), c.low.data(),
                                                           nullptr, c.aln.data(), c.orient.data())
                                : spdp_align_s_seeded(ctx, sc, &spx, c.probs.data(), m, c.hl.data(), c.hn.data(), c.low.data(), nullptr, c.aln.data());
        if (rc >= 0 && ori == 3) for (int k = 0; k < m; ++k) if (c.orient[k]) c.probs[k] = c.probs[m + k];     // rescoring reads the pair that was aligned
        return rc;
    }
    int rescore(Chunk<Problem>& c) { return spdp_skl_rng_s(ctx, sc, rp, c.probs.data(), c.m, c.aln.data(), c.res.data()); }
    void rows(const Chunk<Problem>& c, int k, LocusOut& o)
    {
        const SpdpLocus& L = c.loci[k];
        const SpdpRescored& R = c.res[k];
        const int q_rev = c.orient[k];
        const int rvs = q_rev ? !L.rvs : (L.rvs != 0);                                            // the strand the aligned region lies on
        const int a_len = c.probs[k].a_len;
        o.g.chr = L.chr; o.g.rvs = rvs; o.g.q_rev = q_rev; o.g.score = R.score; o.g.val = R.val;
        std::vector<SpdpMapExon>& ex = o.ex;
        auto site = [&L, rvs](int pos) { return L.base + (rvs ? L.len - pos : pos + 1); };      // Seq::SiteNo
        // positions of the query as given (Seq::SiteNo with inex.sens reversed): the reverse leg turned it, and so did the
        // preparation of a query with a T head -- both: as given again
        const bool turned = (q_rev != 0) != prep_turned(L.query);
        for (int e = 0; e < R.n_exons; ++e) {
            const SpdpExon& x = R.exons[e];
            if (x.left > (1 << 30)) continue;                                                     // (the closing record of the list)
            // the query range covered, from the first exon's rleft to the last one's rright; the reverse leg's turned back
            const int32_t xl = q_rev ? a_len - x.rright : x.rleft, xr = q_rev ? a_len - x.rleft : x.rright;
            o.rleft = ex.empty() ? xl : std::min(o.rleft, xl); o.rright = ex.empty() ? xr : std::max(o.rright, xr);
            if (turned) ex.push_back({a_len - x.rleft, a_len - x.rright + 1, site(x.left), site(x.right - 1)});
            else ex.push_back({x.rleft + 1, x.rright, site(x.left), site(x.right - 1)});
        }
    }
};

// ---- protein queries: the region as the aligner reads it (other strand, Seq::nuc2tron) and its SGPT6 signals (spdp_signals_h),
// spdp_align_h_seeded with the library's own HSP searches, spdp_skl_rng_h.  No orientation, no preparation
struct KindH : ChainBase {
    using Problem = SpdpProblemH;
    using Job = SigJobH;
    // staging block: tron codes | sig5 sig3 sigS sigT sigE (int16) | phs5 phs3 (int8) | dinc, on the device | cano behind them;
    // len + 3 positions per locus
    static constexpr int host_bytes = 14, dev_bytes = 15, pad = 3;
    static constexpr size_t default_mpos = 512;
    const SpdpScoringH* sc; const SpdpSignalModelH* sigmodel; const SpdpRescoreParamsH* rp;
    SpdpScoring costs;                                  // (the gap and intron prices the HSP chaining of the block search reads)
    KindH(const ChainBase& b, const SpdpScoringH* sc_, const SpdpSignalModelH* sm, const SpdpRescoreParamsH* rp_)
        : ChainBase(b), sc(sc_), sigmodel(sm), rp(rp_) {}
    const int32_t* tlen() const { return nullptr; }
    bool prep_turned(int) const { return false; }
    int slots() const { return 1; }
    const SpdpScoring* chain_costs()
    {
        memset(&costs, 0, sizeof costs);
        costs.gop = sc->gop; costs.gep = sc->gep; costs.lgop = sc->lgop; costs.lgep = sc->lgep; costs.codonk1 = sc->codonk1;
        costs.intpen = sc->intpen; costs.intpen_len = sc->intpen_len;
        return &costs;
    }
    int refused()
    {
        if (!sp->wilip || sp->wilip->dvsp != 1) return refuse("SpdpSeedParams.wilip must be the protein model (dvsp = 1)");
        if (!sc->intpen || sc->intpen_len <= 0) return refuse("SpdpScoringH.intpen missing");
        return 0;
    }
    int prepare() { return 0; }

    template <class X> static void lay(X& x, uint8_t* B, int64_t T, int64_t at)
    {
        x.sig5 = (int16_t*) (B + T) + at; x.sig3 = (int16_t*) (B + 3 * T) + at; x.sigS = (int16_t*) (B + 5 * T) + at;
        x.sigT = (int16_t*) (B + 7 * T) + at; x.sigE = (int16_t*) (B + 9 * T) + at;
        x.phs5 = (int8_t*) (B + 11 * T) + at; x.phs3 = (int8_t*) (B + 12 * T) + at; x.dinc = B + 13 * T + at;
    }
    void cut(Chunk<Problem>& c, int j)
    {
        const SpdpLocus& L = c.loci[j];
        uint8_t* dst = c.H + c.at[j];
        spdp_region::materialize_into(genome->codes, genome->chr_off, L.chr, L.base, L.len, L.rvs != 0, true, dst);
        dst[L.len + 1] = dst[L.len + 2] = 0;
    }
    int signals(Chunk<Problem>& c, const std::vector<Job>& jobs, uint8_t* D)
    {
        SignalArgsH A;
        memset(&A, 0, sizeof A);
        A.codes = D; A.cano = D + 14 * c.T;
        lay(A, D, c.T, 0);
        return spdh_signals_run(ctx, sigmodel, jobs, A, 0);
    }
    void point(Chunk<Problem>& c, int j, Problem& P)
    {
        lay(P, c.H, c.T, c.at[j]);
        P.exin_left = c.loci[j].left; P.exin_right = c.loci[j].right;
    }
    int walk(Chunk<Problem>& c)
    {
        const int rc = spdp_align_h_seeded(ctx, sc, sp, c.probs.data(), c.m, c.hl.data(), c.hn.data(), c.low.data(), nullptr, c.aln.data());
        if (rc < 0) return rc;
        // the phases of the junctions the walks chose themselves: where the reference's walk writes into its Exinon (skl_rngH_ng
        // reads them)
        int8_t* phs5 = (int8_t*) (c.H + 11 * c.T); int8_t* phs3 = (int8_t*) (c.H + 12 * c.T);
        for (int j = 0; j < c.m; ++j) {
            const SpdpPhaseMark* mk = nullptr;
            const int nm = spdp_seeded_phase_marks(ctx, j, &mk);
            for (int i = 0; i < nm; ++i) {
                if (mk[i].n < 0 || mk[i].n > c.loci[j].len + 2) continue;
                (mk[i].side == 5 ? phs5 : phs3)[c.at[j] + mk[i].n] = mk[i].value;
            }
        }
        return rc;
    }
    int rescore(Chunk<Problem>& c) { return spdp_skl_rng_h(ctx, sc, rp, c.probs.data(), c.m, c.aln.data(), c.res.data()); }
    void rows(const Chunk<Problem>& c, int k, LocusOut& o)
    {
        const SpdpLocus& L = c.loci[k];
        const SpdpRescored& R = c.res[k];
        const int rvs = L.rvs != 0;
        o.g.chr = L.chr; o.g.rvs = rvs; o.g.q_rev = 0; o.g.score = R.score; o.g.val = R.val;
        std::vector<SpdpMapExon>& ex = o.ex;
        auto site = [&L, rvs](int pos) { return L.base + (rvs ? L.len - pos : pos + 1); };      // Seq::SiteNo
        // an exon closes at a record that carries an intron score; records of frame shifts inside it (iscr = NEVSEL, skl_rngH_ng:
        // src/fwd2h1.cc:739-751, 783-797) do not: the printer reads the exon across them (src/sqpr.cc:896-952, spdp_exon_form)
        int open = -1;
        for (int e = 0; e < R.n_exons; ++e) {
            const SpdpExon& x = R.exons[e];
            if (x.left > (1 << 30)) continue;                                                     // (the closing record of the list)
            if (open < 0) open = e;
            if (ex.empty() && open == e) o.rleft = x.rleft;                                       // the query range covered: every record counts
            o.rright = x.rright;
            if (x.iscr <= SPDP_NEVSEL) continue;
            const SpdpExon& x0 = R.exons[open];
            ex.push_back({x0.rleft + 1, x.rright, site(x0.left), site(x.right - 1)});
            open = -1;
        }
    }
};

// The chain in its steps: setup() checks the arguments and prepares the queries, find() is the block search on one range per
// query, align() takes loci through regions + signals, the seeded walks and the rescoring and hands each to the sink.  The plain
// entries run the steps once (run_once); the dispersed entries run find() per pass and align() per round.
template <class K>
struct Chain : K {
    using K::K;
    using Problem = typename K::Problem;

    // -1: refused (ctx->err says why); 0: go on (n <= 0: there is nothing to do)
    int setup()
    {
        K& R = *this;
        if (!R.ix || !R.hix || !R.genome || !R.sc || !R.sp || !R.sigmodel || !R.fprm || !R.rp || !R.codes || !R.offs) return R.refuse("null argument");
        if (R.refused()) return -1;
        if (R.n <= 0) return 0;
        auto t0 = std::chrono::steady_clock::now();
        R.ql.assign(R.n, 0); R.qr.resize(R.n);
        for (int i = 0; i < R.n; ++i) R.qr[i] = (int32_t) (R.offs[i + 1] - R.offs[i]);
        if (R.prepare()) return -1;
        R.sec[0] += since(t0);
        return 0;
    }

    // the block search for m queries laid out by cd / of (the call's own, or a pass's selection of them), each on its range
    int find(const uint8_t* cd, const int64_t* of, const int32_t* left, const int32_t* right, const int32_t* tl, int32_t m,
             SpdpLocus** loci, int32_t* n_loci, SpdpJuxt** hsps)
    {
        K& R = *this;
        auto t0 = std::chrono::steady_clock::now();
        const int rc = spdp_blk_find_tlen(R.ctx, R.ix, R.hix, R.genome, R.sp->wilip, R.chain_costs(), R.fprm, cd, of, left, right, tl, m, loci, n_loci, hsps, nullptr);
        R.sec[0] += since(t0);
        return rc;
    }

    // loci[k].query: a query of the call; rng (may be null): the query range locus k is aligned on, rng[2 k] .. rng[2 k + 1] of the
    // normalised query (protein: in residues) -- without it the query's own range.  The sink gets every locus, in the order given.
    int align(const SpdpLocus* loci, int n_loci, const SpdpJuxt* hsps, const int32_t* rng, const LocusSink& sink)
    {
        K& R = *this;
        SpdpContext* ctx = R.ctx;
        const SpdpGenome* genome = R.genome;
        const bool verbose = getenv("SPDP_MAP_VERBOSE") != nullptr;
        const int slots = R.slots();
        std::vector<int64_t> positions(n_loci);
        for (int k = 0; k < n_loci; ++k) {
            const SpdpLocus& L = loci[k];
            if (L.chr < 0 || L.chr >= genome->n_chr || L.base < 0 || L.len < 0 || L.left < 0 || L.right > L.len || L.right < L.left ||
                genome->chr_off[L.chr] + L.base + L.len > genome->chr_off[L.chr + 1]) return R.refuse("a locus outside its chromosome");
            positions[k] = slots * (int64_t) (L.len + K::pad);
        }
        // positions (NOT bytes) of the loci one chunk may hold; the arrays of a chunk take host_bytes per position of pinned host
        // memory and dev_bytes on the device, allocated as the chunk needs them.  SPDP_MAP_CHUNK_MPOS = n: n x 2^20 positions
        // (SPDP_MAP_CHUNK_MB: its old name)
        size_t chunk_positions = K::default_mpos << 20;
        for (const char* v : {"SPDP_MAP_CHUNK_MB", "SPDP_MAP_CHUNK_MPOS"})
            if (const char* e = getenv(v)) chunk_positions = (size_t) std::max(1, atoi(e)) << 20;
        (void) hipSetDevice(ctx->device);
        const std::vector<int> bounds = cut_chunks(positions, (int64_t) chunk_positions);
        for (size_t ci = 0; ci + 1 < bounds.size(); ++ci) {
            auto t0 = std::chrono::steady_clock::now();
            const int c0 = bounds[ci], m = bounds[ci + 1] - c0;
            Chunk<Problem> c(loci + c0, m, slots, rng ? rng + 2 * c0 : nullptr);
            for (int k = 0; k < m; ++k) {
                c.at[k] = c.tot; c.tot += positions[c0 + k];
                if (slots == 2) c.at[m + k] = c.at[k] + loci[c0 + k].len + K::pad;
            }
            // ---- the regions as the aligner reads them, then their signals in one launch
            c.T = (c.tot + 255) / 256 * 256;
            c.H = (uint8_t*) ctx->staging(2, (size_t) c.T * K::host_bytes);
            if (!c.H) return R.refuse("no pinned host memory for a chunk's regions and signals (SPDP_MAP_CHUNK_MPOS sets the chunk size)");
            on_host_threads(c.ns, [&](int j) { R.cut(c, j); });
            const double t_regions = since(t0);
            {
                DevMem d;
                HIPCHK(d.get((size_t) c.T * K::dev_bytes));
                uint8_t* D = d.as<uint8_t>();
                HIPCHK(hipMemcpyAsync(D, c.H, c.tot, hipMemcpyHostToDevice, ctx->stream));
                std::vector<typename K::Job> jobs(c.ns);
                for (int j = 0; j < c.ns; ++j) {
                    typename K::Job& J = jobs[j];
                    memset(&J, 0, sizeof J);
                    J.b_off = c.at[j]; J.out_off = c.at[j]; J.b_len = c.locus(j).len; J.left = c.left(j); J.right = c.right(j);
                }
                if (R.signals(c, jobs, D)) return -1;
                HIPCHK(hipMemcpy(c.H + c.T, D + c.T, (size_t) c.T * (K::host_bytes - 1), hipMemcpyDeviceToHost));
            }
            if (verbose) fprintf(stderr, "[map] regions cut %.3f s, signals made and brought back %.3f s\n", t_regions, since(t0) - t_regions);
            for (int j = 0; j < c.ns; ++j) {
                const int k = j < m ? j : j - m;
                const SpdpLocus& L = loci[c0 + k];
                Problem& P = c.probs[j];
                P.a = R.codes + R.offs[L.query]; P.a_len = (int32_t) (R.offs[L.query + 1] - R.offs[L.query]);
                P.b = c.H + c.at[j]; P.b_len = L.len;
                P.b_left = c.left(j); P.b_right = c.right(j);
                // the query's range: the one given for this locus, else its own (the reverse leg: Seq::comrev mirrors it, Seq::rev_attr)
                const int32_t al = c.rng ? c.rng[2 * k] : R.ql[L.query], ar = c.rng ? c.rng[2 * k + 1] : R.qr[L.query];
                P.a_left = j < m ? al : P.a_len - ar; P.a_right = j < m ? ar : P.a_len - al;
                P.a_exgl = P.a_exgr = P.b_exgl = P.b_exgr = 1;
                R.point(c, j, P);
                if (j < m) { c.hl[k] = hsps + L.hsp_off; c.hn[k] = L.n_hsp; }
            }
            R.sec[1] += since(t0);
            // ---- the aligner on every locus, then the printer's scores
            t0 = std::chrono::steady_clock::now();
            const int rc = R.walk(c);
            if (rc < 0) return -1;
            if (rc > 0) ++R.partial;
            R.sec[2] += since(t0);
            if (verbose) {
                int64_t st[12] = {0};
                spdp_seeded_stats(ctx, st, 11);
                fprintf(stderr, "[map] chunk of %d loci, %.1f M positions: regions + signals %.3f s; seeded call %.3f s (upload %.3f, walks with the device idle %.3f, "
                        "device batches %.3f, handing back %.3f; %lld batches, %lld + %lld DP requests, %lld HSP searches)\n", m, c.tot / 1e6, R.sec[1], since(t0),
                        st[6] / 1e6, st[7] / 1e6, st[8] / 1e6, st[9] / 1e6, (long long) st[0], (long long) st[1], (long long) st[2], (long long) st[4]);
            }
            t0 = std::chrono::steady_clock::now();
            if (R.rescore(c)) return -1;
            for (int k = 0; k < m; ++k) {
                LocusOut o;
                o.aligned = c.aln[k].n_skl >= 1;
                o.g = no_gene();
                if (o.aligned) R.rows(c, k, o);
                sink(loci[c0 + k], std::move(o));
            }
            R.sec[3] += since(t0);
        }
        return 0;
    }

    int finish(double* seconds)
    {
        K& R = *this;
        if (seconds) memcpy(seconds, R.sec, sizeof R.sec);
        if (R.partial) { R.refuse("some walks met a state the seeded path does not serve; those loci come back without an alignment"); return 1; }
        return 0;
    }
};
using ChainS = Chain<KindS>;
using ChainH = Chain<KindH>;

// the steps once, every locus to the sink: -1, 0, or 1 (some loci came back without an alignment)
template <class Chain>
int run_once(Chain& R, const LocusSink& sink, double* seconds)
{
    if (R.setup()) return -1;
    if (R.n <= 0) return 0;
    SpdpLocus* loci = nullptr; SpdpJuxt* hsps = nullptr; int32_t n_loci = 0;
    if (R.find(R.codes, R.offs, R.ql.data(), R.qr.data(), R.tlen(), R.n, &loci, &n_loci, &hsps)) return -1;
    struct Owned { SpdpLocus* l; SpdpJuxt* h; ~Owned() { free(l); free(h); } } owned{loci, hsps};
    if (R.align(loci, n_loci, hsps, nullptr, sink)) return -1;
    return R.finish(seconds);
}

}  // namespace

// ---- dispersed loci: quick4 around blkaln with algmode.mlt = 1 (`spaln -pr`; include/spdp.h "dispersed loci") ---------------------
// quick4's rule alone (src/spaln.cc:1114-1134): which stretches of the query's range are searched again after its first search
// left the range at cov.  Both comparisons are strict.
extern "C" int spdp_dispersed_rests(const int32_t org[2], const int32_t cov[2], int32_t min_seg_len, int32_t rests[4])
{
    if (!org || !cov || !rests) return -1;
    int k = 0;
    if (cov[0] - org[0] > min_seg_len) { rests[0] = org[0]; rests[1] = cov[0]; ++k; }
    if (org[1] - cov[1] > min_seg_len) { rests[2 * k] = cov[1]; rests[2 * k + 1] = org[1]; ++k; }
    return k;
}

namespace {

// one search of quick4: query q on [l, r) of its normalised form; part: 0 the first search, 1 the left rest, 2 the right rest
struct Piece { int q; int32_t l, r; int part; };
// what blkaln leaves of it: every locus as it was aligned, in the block search's order, and the range the query has afterwards
struct PieceOut { std::vector<LocusOut> loci; int32_t l, r; };

// One pass = blkaln for every piece: the block search on the pieces' ranges, then the loci by rounds.  blkaln aligns a query's
// loci one after the other and narrows the query to what a locus covered once that locus passed the threshold (src/spaln.cc:914-918,
// 950-954), so locus k + 1 is aligned on the range locus k left -- with the HSPs found on the range before.  A round aligns, for
// every piece, all loci not yet settled on the piece's range as it stands; they are settled in order up to and including the
// first one that changes the range, the others wait for the next round.  Most pieces have one locus, and a locus that covers the
// whole range changes nothing: such pieces are done in one round (a round costs a chain of request latencies).
template <class Chain>
int dispersed_pass(Chain& R, const std::vector<Piece>& pieces, bool whole_call, int vthr, std::vector<PieceOut>& out)
{
    const int m = (int) pieces.size();
    out.assign(m, PieceOut());
    if (!m) return 0;
    std::vector<int32_t> l(m), r(m), tl;
    for (int p = 0; p < m; ++p) { out[p].l = l[p] = pieces[p].l; out[p].r = r[p] = pieces[p].r; }
    // the queries of the pass as the block search takes them: the call's own (the first pass: piece p is query p), or the whole
    // queries of the pieces one behind the other -- a rest is a range of its query, so every position keeps its meaning.  That is a
    // host copy of each such query (twice for a query with two rests) and the upload of whole queries for what may be short
    // rests: spdp_blk_find takes queries that lie one behind the other, and has no indirection that would let two pieces share one
    const uint8_t* cd = R.codes; const int64_t* of = R.offs;
    std::vector<uint8_t> sel; std::vector<int64_t> sel_off;
    if (!whole_call) {
        sel_off.assign(m + 1, 0);
        for (int p = 0; p < m; ++p) sel_off[p + 1] = sel_off[p] + (R.offs[pieces[p].q + 1] - R.offs[pieces[p].q]);
        sel.resize((size_t) sel_off[m]);
        for (int p = 0; p < m; ++p) memcpy(sel.data() + sel_off[p], R.codes + R.offs[pieces[p].q], (size_t) (sel_off[p + 1] - sel_off[p]));
        cd = sel.data(); of = sel_off.data();
    }
    if (R.tlen()) { tl.resize(m); for (int p = 0; p < m; ++p) tl[p] = R.tlen()[pieces[p].q]; }
    SpdpLocus* loci = nullptr; SpdpJuxt* hsps = nullptr; int32_t n_loci = 0;
    if (R.find(cd, of, l.data(), r.data(), tl.empty() ? nullptr : tl.data(), m, &loci, &n_loci, &hsps)) return -1;
    struct Owned { SpdpLocus* l; SpdpJuxt* h; ~Owned() { free(l); free(h); } } owned{loci, hsps};
    std::vector<int> end(m + 1, 0);                     // piece p's loci: loci[end[p] .. end[p + 1]), as findblock listed them
    for (int k = 0; k < n_loci; ++k) ++end[loci[k].query + 1];
    for (int p = 0; p < m; ++p) end[p + 1] += end[p];
    for (int k = 0; k < n_loci; ++k) loci[k].query = pieces[loci[k].query].q;
    std::vector<int> next(end.begin(), end.end() - 1);
    int rounds = 0;
    size_t aligned = 0;
    for (;; ++rounds) {
        std::vector<SpdpLocus> batch;
        std::vector<int32_t> rng;
        for (int p = 0; p < m; ++p)
            for (int k = next[p]; k < end[p + 1]; ++k) { batch.push_back(loci[k]); rng.push_back(out[p].l); rng.push_back(out[p].r); }
        if (batch.empty()) break;
        aligned += batch.size();
        std::vector<LocusOut> got;
        got.reserve(batch.size());
        if (R.align(batch.data(), (int) batch.size(), hsps, rng.data(), [&got](const SpdpLocus&, LocusOut&& o) { got.push_back(std::move(o)); })) return -1;
        size_t j = 0;
        for (int p = 0; p < m; ++p) {
            const int waiting = end[p + 1] - next[p];
            for (int i = 0; i < waiting; ++i) {
                LocusOut& o = got[j + i];
                const bool narrows = o.aligned && o.g.score > vthr && (o.rleft != out[p].l || o.rright != out[p].r);
                const int32_t nl = o.rleft, nr = o.rright;
                out[p].loci.push_back(std::move(o));
                ++next[p];
                if (narrows) { out[p].l = nl; out[p].r = nr; break; }       // (the loci behind it were aligned on a range that is gone)
            }
            j += waiting;
        }
    }
    if (getenv("SPDP_MAP_VERBOSE")) fprintf(stderr, "[dispersed] pass of %d searches: %d loci, %d rounds, %zu alignments\n", m, n_loci, rounds, aligned);
    return 0;
}

// quick4 for every query of the call (src/spaln.cc:1114-1134): the first search on the query's own range, then in one further
// pass every rest that is longer than min_seg_len; per search the locus blkaln prints with MaxOut = 1
template <class Chain>
int dispersed(Chain& R, int32_t min_seg_len, int64_t* gene_off, SpdpMapGene** genes, SpdpMapExon** exons, int32_t** part, int32_t* covered)
{
    const int n = R.n;
    const int vthr = R.sp->vthr;
    std::vector<Piece> first(n), rest;
    for (int q = 0; q < n; ++q) first[q] = {q, R.ql[q], R.qr[q], 0};
    std::vector<PieceOut> o1, o2;
    if (dispersed_pass(R, first, true, vthr, o1)) return -1;
    for (int q = 0; q < n; ++q) {
        const int32_t org[2] = {R.ql[q], R.qr[q]}, cov[2] = {o1[q].l, o1[q].r};
        // (blkaln's return value: 0 only when findblock found nothing -- the range is then as it was, and nothing is left over)
        int32_t rests[4];
        const int nr = o1[q].loci.empty() ? 0 : spdp_dispersed_rests(org, cov, min_seg_len, rests);
        // (which rest it is stands in the rest itself: the left one begins where the query's range begins and ends where cov begins)
        for (int k = 0; k < nr; ++k) rest.push_back({q, rests[2 * k], rests[2 * k + 1], rests[2 * k] == org[0] && rests[2 * k + 1] == cov[0] ? 1 : 2});
        if (covered) {                                  // in the positions of the query as given: the preparation may have turned it
            const int32_t len = (int32_t) (R.offs[q + 1] - R.offs[q]);
            covered[2 * q] = R.prep_turned(q) ? len - cov[1] : cov[0];
            covered[2 * q + 1] = R.prep_turned(q) ? len - cov[0] : cov[1];
        }
    }
    if (dispersed_pass(R, rest, false, vthr, o2)) return -1;
    Reported rep(n);
    std::vector<std::vector<int32_t>> parts(n);
    auto report = [&](const Piece& pc, PieceOut& po) {
        const size_t before = rep.genes[pc.q].size();
        select_printed(po.loci, 1, 0, vthr, rep.genes[pc.q], rep.ex[pc.q]);
        parts[pc.q].resize(parts[pc.q].size() + (rep.genes[pc.q].size() - before), pc.part);
    };
    for (int q = 0; q < n; ++q) report(first[q], o1[q]);
    for (size_t k = 0; k < rest.size(); ++k) report(rest[k], o2[k]);       // (a query's left rest stands before its right one)
    if (hand_out(R.ctx, R.who, rep, n, gene_off, genes, exons)) return -1;
    *part = (int32_t*) malloc(sizeof(int32_t) * std::max<size_t>((size_t) gene_off[n], 1));
    if (!*part) return R.refuse("out of memory");
    size_t k = 0;
    for (int q = 0; q < n; ++q) for (int32_t v : parts[q]) (*part)[k++] = v;
    return 0;
}

// what both dispersed entries refuse before anything is launched
int check_dispersed(SpdpContext* ctx, const char* who, const SpdpBlkFindParams* fprm, const SpdpSeedParams* sp, int32_t min_seg_len)
{
    if (!fprm || !sp) { ctx->err = std::string(who) + ": null argument"; return -1; }
    if (min_seg_len <= 0) { ctx->err = std::string(who) + ": min_seg_len must be > 0 (the program's MinSegLen = 2 Ktuple + Nshift of the index)"; return -1; }
    if (fprm->max_out != 1) { ctx->err = std::string(who) + ": max_out must be 1 (-pr together with -M N is another mode)"; return -1; }
    return 0;
}

// The frame of every entry: `needed` are the pointers the entry itself reads (the outputs among them), `outs` those of them it
// hands memory out through -- nulled first, freed and nulled again on every failing path, so that a failed call hands nothing out.
// body() gives the entry's return code.  Nothing of C++ crosses the C boundary.
template <class Body>
int entry(SpdpContext* ctx, const char* who, std::initializer_list<const void*> needed, std::initializer_list<void**> outs, Body body)
{
    if (!ctx) return -1;
    for (const void* p : needed) if (!p) { ctx->err = std::string(who) + ": null argument"; return -1; }
    for (void** p : outs) *p = nullptr;
    int rc = -1;
    try { rc = body(); }
    catch (const std::bad_alloc&) { ctx->err = std::string(who) + ": out of host memory (SPDP_MAP_CHUNK_MPOS sets the size of a chunk)"; }
    if (rc < 0) for (void** p : outs) { free(*p); *p = nullptr; }
    return rc;
}

// the two sinks around run_once: the best locus per query into genes[n], and the list spaln -M prints
template <class Chain>
int best_only(Chain& R, SpdpMapGene* genes, SpdpMapExon** exons, double* seconds)
{
    const int n = R.n;
    BestSink best(std::max(n, 0));
    for (int i = 0; i < n; ++i) genes[i] = best.best[i];
    const int rc = run_once(R, std::ref(best), seconds);
    if (rc < 0 || n <= 0) return rc;
    return best.finish(R.ctx, R.who, n, genes, exons) ? -1 : rc;
}
template <class Chain>
int printed_lists(Chain& R, int32_t all_out, int64_t* gene_off, SpdpMapGene** genes, SpdpMapExon** exons, double* seconds)
{
    if (check_multi(R.ctx, R.who, R.hix, R.fprm)) return -1;
    const int n = std::max(R.n, 0);
    MultiSink multi(n, R.fprm->max_out, all_out, R.sp->vthr);
    const int rc = run_once(R, std::ref(multi), seconds);
    if (rc < 0) return rc;
    return multi.finish(R.ctx, R.who, n, gene_off, genes, exons) ? -1 : rc;
}
template <class Chain>
int dispersed_lists(Chain& R, int32_t min_seg_len, int64_t* gene_off, SpdpMapGene** genes, SpdpMapExon** exons, int32_t** part, int32_t* covered,
                    double* seconds)
{
    if (check_dispersed(R.ctx, R.who, R.fprm, R.sp, min_seg_len)) return -1;
    R.n = std::max(R.n, 0);
    if (R.setup()) return -1;
    if (dispersed(R, min_seg_len, gene_off, genes, exons, part, covered)) return -1;
    return R.finish(seconds);
}

}  // namespace

// (every entry: what it was handed, as the chain holds it)
#define CHAIN_BASE(who) ChainBase{who, ctx, ix, hix, genome, sp, fprm, codes, offs, n}

extern "C" int spdp_map_align_s(SpdpContext* ctx, const SpdpBlkIndex* ix, const SpdpBlkIndexDesc* hix, const SpdpGenome* genome,
    const SpdpScoring* sc, const SpdpSeedParams* sp, const SpdpSignalModel* sigmodel, const SpdpBlkFindParams* fprm, const SpdpRescoreParams* rp,
    const uint8_t* codes, const int64_t* offs, int32_t n,
    int32_t ori, SpdpMapGene* genes, SpdpMapExon** exons, double* seconds)
{
    const char* who = "spdp_map_align_s";
    return entry(ctx, who, {genes, exons}, {(void**) exons}, [&] {
        ChainS R(CHAIN_BASE(who), sc, sigmodel, rp, ori);
        return best_only(R, genes, exons, seconds);
    });
}

extern "C" int spdp_map_align_s_multi(SpdpContext* ctx, const SpdpBlkIndex* ix, const SpdpBlkIndexDesc* hix, const SpdpGenome* genome,
    const SpdpScoring* sc, const SpdpSeedParams* sp, const SpdpSignalModel* sigmodel, const SpdpBlkFindParams* fprm, const SpdpRescoreParams* rp,
    const uint8_t* codes, const int64_t* offs, int32_t n,
    int32_t ori, int32_t all_out, int64_t* gene_off, SpdpMapGene** genes, SpdpMapExon** exons,
                                      double* seconds)
{
    const char* who = "spdp_map_align_s_multi";
    return entry(ctx, who, {gene_off, genes, exons, sp}, {(void**) genes, (void**) exons}, [&] {
        ChainS R(CHAIN_BASE(who), sc, sigmodel, rp, ori);
        return printed_lists(R, all_out, gene_off, genes, exons, seconds);
    });
}

// ---- protein queries against the translated index
extern "C" int spdp_map_align_h(SpdpContext* ctx, const SpdpBlkIndex* ix, const SpdpBlkIndexDesc* hix, const SpdpGenome* genome,
    const SpdpScoringH* sc, const SpdpSeedParams* sp, const SpdpSignalModelH* sigmodel, const SpdpBlkFindParams* fprm, const SpdpRescoreParamsH* rp,
    const uint8_t* codes, const int64_t* offs, int32_t n,
    SpdpMapGene* genes, SpdpMapExon** exons, double* seconds)
{
    const char* who = "spdp_map_align_h";
    return entry(ctx, who, {genes, exons}, {(void**) exons}, [&] {
        ChainH R(CHAIN_BASE(who), sc, sigmodel, rp);
        return best_only(R, genes, exons, seconds);
    });
}

extern "C" int spdp_map_align_h_multi(SpdpContext* ctx, const SpdpBlkIndex* ix, const SpdpBlkIndexDesc* hix, const SpdpGenome* genome,
    const SpdpScoringH* sc, const SpdpSeedParams* sp, const SpdpSignalModelH* sigmodel, const SpdpBlkFindParams* fprm, const SpdpRescoreParamsH* rp,
    const uint8_t* codes, const int64_t* offs, int32_t n,
    int32_t all_out, int64_t* gene_off, SpdpMapGene** genes, SpdpMapExon** exons, double* seconds)
{
    const char* who = "spdp_map_align_h_multi";
    return entry(ctx, who, {gene_off, genes, exons, sp}, {(void**) genes, (void**) exons}, [&] {
        ChainH R(CHAIN_BASE(who), sc, sigmodel, rp);
        return printed_lists(R, all_out, gene_off, genes, exons, seconds);
    });
}

// ---- the cDNA entries with the query preparation in front (include/spdp.h "query preparation")
extern "C" int spdp_map_align_s_prep(SpdpContext* ctx, const SpdpBlkIndex* ix, const SpdpBlkIndexDesc* hix, const SpdpGenome* genome,
    const SpdpScoring* sc, const SpdpSeedParams* sp, const SpdpSignalModel* sigmodel, const SpdpBlkFindParams* fprm, const SpdpRescoreParams* rp,
    const uint8_t* codes, const int64_t* offs, int32_t n,
    const SpdpQueryPrep* prep, SpdpMapGene* genes, SpdpMapExon** exons, double* seconds,
                                     SpdpQueryTail* tails)
{
    const char* who = "spdp_map_align_s_prep";
    return entry(ctx, who, {genes, exons}, {(void**) exons}, [&] {
        ChainS R(CHAIN_BASE(who), sc, sigmodel, rp, 0, prep, true, tails);
        return best_only(R, genes, exons, seconds);
    });
}

extern "C" int spdp_map_align_s_multi_prep(SpdpContext* ctx, const SpdpBlkIndex* ix, const SpdpBlkIndexDesc* hix, const SpdpGenome* genome,
    const SpdpScoring* sc, const SpdpSeedParams* sp, const SpdpSignalModel* sigmodel, const SpdpBlkFindParams* fprm, const SpdpRescoreParams* rp,
    const uint8_t* codes, const int64_t* offs, int32_t n,
    const SpdpQueryPrep* prep, int32_t all_out, int64_t* gene_off, SpdpMapGene** genes,
                                           SpdpMapExon** exons, double* seconds, SpdpQueryTail* tails)
{
    const char* who = "spdp_map_align_s_multi_prep";
    return entry(ctx, who, {gene_off, genes, exons, sp}, {(void**) genes, (void**) exons}, [&] {
        ChainS R(CHAIN_BASE(who), sc, sigmodel, rp, 0, prep, true, tails);
        return printed_lists(R, all_out, gene_off, genes, exons, seconds);
    });
}

// ---- dispersed loci (`spaln -pr`)
extern "C" int spdp_map_align_s_dispersed(SpdpContext* ctx, const SpdpBlkIndex* ix, const SpdpBlkIndexDesc* hix, const SpdpGenome* genome,
    const SpdpScoring* sc, const SpdpSeedParams* sp, const SpdpSignalModel* sigmodel, const SpdpBlkFindParams* fprm, const SpdpRescoreParams* rp,
    const uint8_t* codes, const int64_t* offs, int32_t n,
    int32_t ori, const SpdpQueryPrep* prep, int32_t min_seg_len, int64_t* gene_off,
                                          SpdpMapGene** genes, SpdpMapExon** exons, int32_t** part, int32_t* covered, double* seconds,
                                          SpdpQueryTail* tails)
{
    const char* who = "spdp_map_align_s_dispersed";
    return entry(ctx, who, {gene_off, genes, exons, part}, {(void**) genes, (void**) exons, (void**) part}, [&] {
        ChainS R(CHAIN_BASE(who), sc, sigmodel, rp, ori, prep, prep != nullptr, tails);
        return dispersed_lists(R, min_seg_len, gene_off, genes, exons, part, covered, seconds);
    });
}

extern "C" int spdp_map_align_h_dispersed(SpdpContext* ctx, const SpdpBlkIndex* ix, const SpdpBlkIndexDesc* hix, const SpdpGenome* genome,
    const SpdpScoringH* sc, const SpdpSeedParams* sp, const SpdpSignalModelH* sigmodel, const SpdpBlkFindParams* fprm, const SpdpRescoreParamsH* rp,
    const uint8_t* codes, const int64_t* offs, int32_t n,
    int32_t min_seg_len, int64_t* gene_off, SpdpMapGene** genes, SpdpMapExon** exons,
                                          int32_t** part, int32_t* covered, double* seconds)
{
    const char* who = "spdp_map_align_h_dispersed";
    return entry(ctx, who, {gene_off, genes, exons, part}, {(void**) genes, (void**) exons, (void**) part}, [&] {
        ChainH R(CHAIN_BASE(who), sc, sigmodel, rp);
        return dispersed_lists(R, min_seg_len, gene_off, genes, exons, part, covered, seconds);
    });
}
