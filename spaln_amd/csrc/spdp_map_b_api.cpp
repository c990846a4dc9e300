// spdp_map_b_api.cpp -- protein queries against a protein database in one call (include/spdp.h, spdp_map_align_b): blkaln for AvsA
// (ogotoh/spaln v3.0.7 src/spaln.cc:846-1014).  finds on the device, every candidate a pair, the pairs as one seeded alignment call,
// skl_rngB_ng, the threshold, the insertion sort by fstat.val.  A short chain of its own: it shares no step with the map + align
// chain of the genome entries (spdp_map_api.cpp) -- no loci, no regions, no signals, no chunks that hand the device on.
#include "spdp_internal.h"
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {
double since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); }

}   // namespace

extern "C" int spdp_blk_finds_stats(const SpdpContext* ctx, int64_t* out, int n)
{
    if (!ctx || !out) return -1;
    for (int i = 0; i < n && i < 8; ++i) out[i] = ctx->finds_stats[i];
    return 0;
}

static int map_align_b(SpdpContext* ctx, const SpdpBlkIndex* ix, const SpdpBlkIndexDesc* hix, const SpdpGenome* db,
                       const SpdpScoring* sc, const SpdpUnsplicedParams* up, const SpdpSeedParams* sp, const SpdpBlkFindsParams* fprm,
                       const uint8_t* codes, const int64_t* offs, int32_t n, int32_t all_out,
                       int64_t* hit_off, SpdpMapHitB** hits, SpdpSkl** corners, double* seconds)
{
    const auto t_call = std::chrono::steady_clock::now();
    memset(ctx->finds_stats, 0, sizeof ctx->finds_stats);
    // ---- the queries the program searches: MinQuery = 2 Ktuple + Nshift (SrchBlk::MinQuery, src/blksrc.cc:2015; src/spaln.cc:1087, 1104)
    const int min_query = 2 * hix->bitpat[0] + hix->nshift;
    std::vector<int> asked;
    for (int i = 0; i < n; ++i) {
        if (offs[i + 1] - offs[i] < 0 || offs[i + 1] - offs[i] > INT32_MAX) { ctx->err = "spdp_map_align_b: offs do not ascend"; return -1; }
        if (offs[i + 1] - offs[i] > 65535) { ctx->err = "spdp_map_align_b: a query longer than 65535 residues (a run of the vote counts its words in 16 bits)"; return -1; }
        if (offs[i + 1] - offs[i] >= min_query) asked.push_back(i);
    }
    const int m = (int) asked.size();
    ctx->finds_stats[1] = n - m;
    // ---- finds
    const int out_cap = 6 + 2 * (fprm->max_out + 10) + 1 + fprm->max_out;
    std::vector<int32_t> rec((size_t) std::max(m, 1) * out_cap, 0), left((size_t) std::max(m, 1), 0), right((size_t) std::max(m, 1), 0);
    std::vector<int64_t> qo((size_t) m + 1, 0);
    std::vector<uint8_t> qc;
    for (int k = 0; k < m; ++k) {
        const int i = asked[k];
        qc.insert(qc.end(), codes + offs[i], codes + offs[i + 1]);
        qo[k + 1] = (int64_t) qc.size(); right[k] = (int32_t) (offs[i + 1] - offs[i]);
    }
    float vote_ms = 0.f;
    auto t0 = std::chrono::steady_clock::now();
    if (m && spdp_blk_finds(ctx, ix, hix, fprm, qc.data(), qo.data(), left.data(), right.data(), m, rec.data(), out_cap, &vote_ms)) return -1;
    const double t_vote = since(t0);
    // ---- every candidate a pair: query = a, database sequence = b
    uint8_t exg[4];                                     // a_exgl, a_exgr, b_exgl, b_exgr (src/spaln.cc:865-866, 908-909)
    if (sp->lcl & 16) exg[0] = exg[1] = exg[2] = exg[3] = 1;
    else { exg[0] = (sp->lcl & 4) != 0; exg[1] = (sp->lcl & 8) != 0; exg[2] = (sp->lcl & 1) != 0; exg[3] = (sp->lcl & 2) != 0; }
    std::vector<SpdpProblem> probs;
    std::vector<int> owner, seq_of;
    for (int k = 0; k < m; ++k) {
        const int32_t* r = rec.data() + (size_t) k * out_cap;
        if (r[2] & (SPDP_BLK_CUT | SPDP_BLK_TABLE)) { ctx->err = "spdp_map_align_b: a record of the vote came back cut or the index is malformed (SPDP_BLK_TABLE)"; return -1; }
        if (!(r[2] & SPDP_BLK_REACHED)) { ++ctx->finds_stats[1]; continue; }   // (finds returned ERROR: too short for it)
        ++ctx->finds_stats[0];
        const int sigm = r[5], nc = r[6 + 2 * sigm];
        for (int j = 0; j < nc; ++j) {
            const int c = r[7 + 2 * sigm + j];
            if (c < 0 || c >= db->n_chr) continue;      // (a sequence met before keeps its slot: one block per sequence never gets here)
            const int i = asked[k];
            SpdpProblem p;
            memset(&p, 0, sizeof p);
            p.a = codes + offs[i]; p.a_len = (int32_t) (offs[i + 1] - offs[i]);
            p.b = db->codes + db->chr_off[c]; p.b_len = (int32_t) (db->chr_off[c + 1] - db->chr_off[c]);
            p.a_right = p.a_len; p.b_right = p.b_len;
            p.a_exgl = exg[0]; p.a_exgr = exg[1]; p.b_exgl = exg[2]; p.b_exgr = exg[3];
            probs.push_back(p); owner.push_back(i); seq_of.push_back(c);
        }
    }
    const int np = (int) probs.size();
    ctx->finds_stats[2] = np;
    // ---- one alignment call, then skl_rngB_ng
    t0 = std::chrono::steady_clock::now();
    std::vector<SpdpAlignment> aln((size_t) std::max(np, 1));
    memset(aln.data(), 0, sizeof(SpdpAlignment) * aln.size());
    std::vector<SpdpRescoredB> st((size_t) std::max(np, 1));
    memset(st.data(), 0, sizeof(SpdpRescoredB) * st.size());
    struct Release { std::vector<SpdpAlignment>& a; int n; ~Release() { if (n) spdp_free_alignments(a.data(), n); } } release{aln, 0};
    if (np) {
        int rc;
        if (sp->qck > 0) {
            std::vector<const SpdpJuxt*> no_hsps((size_t) np, nullptr);
            std::vector<int32_t> zero((size_t) np, 0);
            rc = spdp_align_b_seeded(ctx, sc, up, sp, probs.data(), np, no_hsps.data(), zero.data(), zero.data(), nullptr, aln.data());
        } else rc = spdp_align_b(ctx, sc, up, probs.data(), np, aln.data());
        if (rc < 0) return -1;
        release.n = np;
        if (spdp_skl_rng_b(sc, up, probs.data(), np, aln.data(), st.data())) { ctx->err = "spdp_map_align_b: spdp_skl_rng_b refused the alignments"; return -1; }
    }
    const double t_align = since(t0);
    // ---- per query: the threshold, the insertion sort by fstat.val (stable, the first on ties), the first min(MaxOut, kept)
    t0 = std::chrono::steady_clock::now();
    std::vector<SpdpMapHitB> H;
    std::vector<SpdpSkl> C;
    std::vector<int64_t> off((size_t) n + 1, 0);
    int at = 0;
    for (int i = 0; i < n; ++i) {
        off[i] = (int64_t) H.size();
        const int first = at;
        while (at < np && owner[at] == i) ++at;
        const int nparalog = at - first;
        int n_out = 0;
        std::vector<int> odr;
        for (int k = 0; k < nparalog; ++k) {
            const SpdpAlignment& a = aln[first + k];
            const bool has = a.n_skl >= 3 && a.skl;
            const int32_t v = has ? st[first + k].val : 0;
            // (gsinf->scr is what skl_rngB_ng returned by then -- GsI->scr = skl_rngB_ng(..), src/spaln.cc:684; the two-file form compares
            // fstat.val outright, :794 --, not the engine's score: tests/test_gpu_aa_search.py, runs H160 / H270)
            if (has && (all_out || v > sp->vthr)) ++n_out; else if (has) ++ctx->finds_stats[3];
            int pos = (int) odr.size();
            while (pos > 0 && v > ((aln[first + odr[pos - 1]].n_skl >= 3 && aln[first + odr[pos - 1]].skl) ? st[first + odr[pos - 1]].val : 0)) --pos;
            odr.insert(odr.begin() + pos, k);
        }
        n_out = std::min(n_out, (int) fprm->max_out);
        for (int r = 0; r < n_out; ++r) {
            const int k = first + odr[r];
            const SpdpAlignment& a = aln[k];
            if (!(a.n_skl >= 3 && a.skl)) continue;     // (if (!gsinf->skl) continue;)
            const SpdpRescoredB& s = st[k];
            if (s.first < 0 || s.n_trim < 1 || s.first + s.n_trim > a.n_skl) continue;
            SpdpMapHitB h;
            memset(&h, 0, sizeof h);
            h.seq = seq_of[k]; h.score = a.score; h.val = s.val; h.mch = s.mch; h.mmc = s.mmc; h.gap = s.gap; h.unp = s.unp;
            h.n_corners = s.n_trim; h.corner_off = (int64_t) C.size();
            C.insert(C.end(), a.skl + s.first, a.skl + s.first + s.n_trim);
            h.a_left = a.skl[s.first].m; h.b_left = a.skl[s.first].n;
            h.a_right = a.skl[s.first + s.n_trim - 1].m; h.b_right = a.skl[s.first + s.n_trim - 1].n;
            H.push_back(h);
        }
    }
    off[n] = (int64_t) H.size();
    *hits = (SpdpMapHitB*) malloc(sizeof(SpdpMapHitB) * std::max<size_t>(H.size(), 1));
    *corners = (SpdpSkl*) malloc(sizeof(SpdpSkl) * std::max<size_t>(C.size(), 1));
    if (!*hits || !*corners) { free(*hits); free(*corners); *hits = nullptr; *corners = nullptr; ctx->err = "spdp_map_align_b: out of memory"; return -1; }
    if (!H.empty()) memcpy(*hits, H.data(), sizeof(SpdpMapHitB) * H.size());
    if (!C.empty()) memcpy(*corners, C.data(), sizeof(SpdpSkl) * C.size());
    memcpy(hit_off, off.data(), sizeof(int64_t) * off.size());
    const double t_host = since(t0), t_all = since(t_call);
    ctx->finds_stats[4] = (int64_t) (vote_ms * 1e3); ctx->finds_stats[5] = (int64_t) (t_align * 1e6);
    ctx->finds_stats[6] = (int64_t) ((t_all - t_align - vote_ms * 1e-3) * 1e6);
    if (seconds) { seconds[0] = t_vote; seconds[1] = t_align; seconds[2] = t_host; seconds[3] = t_all; }
    return 0;
}

extern "C" int spdp_map_align_b(SpdpContext* ctx, const SpdpBlkIndex* ix, const SpdpBlkIndexDesc* hix, const SpdpGenome* db,
                                const SpdpScoring* sc, const SpdpUnsplicedParams* up, const SpdpSeedParams* sp, const SpdpBlkFindsParams* fprm,
                                const uint8_t* codes, const int64_t* offs, int32_t n, int32_t all_out,
                                int64_t* hit_off, SpdpMapHitB** hits, SpdpSkl** corners, double* seconds)
{
    if (!ctx) return -1;
    if (!ix || !hix || !db || !sc || !up || !sp || !fprm || !hit_off || !hits || !corners || (n > 0 && (!codes || !offs))) { ctx->err = "spdp_map_align_b: null argument"; return -1; }
    *hits = nullptr; *corners = nullptr;
    if (!db->codes || !db->chr_off || !hix->bitpat || hix->n_bitpat < 1) { ctx->err = "spdp_map_align_b: null argument"; return -1; }
    if (hix->drna) { ctx->err = "spdp_map_align_b: a nucleotide index (protein queries search the amino-acid index of a protein database, spaln -W -KA)"; return -1; }
    if (hix->ncand != fprm->max_out + 10) { ctx->err = "spdp_map_align_b: the index was not made for max_out (Ncand != MaxOut + 10, src/blksrc.cc:2220)"; return -1; }
    if (db->n_chr != hix->n_chr) { ctx->err = "spdp_map_align_b: the database's sequence count differs from the index's"; return -1; }
    if (sp->qck > 0) {
        if (const char* why = spdp_align_b_seeded_refusal(sc, up, sp, 0, 0)) { ctx->err = why; return -1; }
    }
    if (n <= 0) { if (n == 0) hit_off[0] = 0; return 0; }
    try { return map_align_b(ctx, ix, hix, db, sc, up, sp, fprm, codes, offs, n, all_out, hit_off, hits, corners, seconds); }
    catch (...) {                                       // (nothing of C++ crosses the C boundary)
        if (*hits) { free(*hits); *hits = nullptr; }
        if (*corners) { free(*corners); *corners = nullptr; }
        ctx->err = "spdp_map_align_b: out of host memory";
        return -1;
    }
}
