// b_seeded_host_check.cpp -- the seeded walk of the unspliced aligner on the CPU, as a program of its own
// (tests/test_b_seeded_host.py builds it with -fsanitize=address,undefined and runs it on a text dump of the fixtures).
//
// It compiles the product's own headers: the walk (spdp_b_seeded_walk.h), the HSP search (spdp_hsp_host.h), the branches of
// lspB_ng without a DP cell (spdp_b_host.h) and what follows a sweep (spdp_b_walk.h: lastB_ng and the record walk).  Only the
// sweep itself is emulated (tests/b_sweep_host.h, shared with b_thin_host_check.cpp): a request of at most 16 rows lane by lane
// the way spdp_b_sweep_thin runs it, with the shared step function thin_step_b; a larger one in the tiled layout, row by row.
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

#include "b_sweep_host.h"
#include "../spaln_amd/csrc/spdp_b_seeded_walk.h"
#include "../spaln_amd/csrc/spdp_hsp_host.h"

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
        int served;
        bool bad;
        const int score = b_sweep_host::request(*sc, tgapf, p, w, true, rec, served, bad);
        ++(served == b_sweep_host::SERVED_THIN ? n_thin : (served == b_sweep_host::SERVED_TILED ? n_wide : n_host));
        if (bad) failed = true;
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
