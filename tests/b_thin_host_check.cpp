// b_thin_host_check.cpp -- single lspB_ng requests of the unspliced aligner on the CPU, as a program of its own
// (tests/test_b_thin_host.py builds it with -fsanitize=address,undefined and feeds it every case of tests/thin_cases.py).
//
// Each request goes the way spdp_lsp_b sends it, with the product's own headers: the window (ladder::stripe<1>, spdp_ladder.h),
// lsp_without_cells and forward_terms (spdp_b_host.h), the sweep emulated in the thin or the tiled layout (tests/b_sweep_host.h:
// thin_step_b, thin_geo_b, thin_top_b and trace_index_b of spdp_b_walk.h), finish_forward_b and close_records.
//
// Input: whitespace-separated records, each led by a letter.
//   S mtx_dim, mtx_dim^2 entries, gop gep lgop lgep codonk1 noll local sh tgapf(float)      the bundle of the cases that follow
//   P a_len b_len, the codes of a and of b                                                  the pair of the cases that follow
//   C id a_left a_right b_left b_right, four end flags (a_exgl a_exgr b_exgl b_exgr), thin_allowed
// Output per case: id, score, which way it was served (0 without a cell, 1 thin, 2 tiled), the number of records, the records.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "b_sweep_host.h"
#include "../spaln_amd/csrc/spdp_ladder.h"

namespace {

int rd(FILE* f)
{
    int v;
    if (fscanf(f, "%d", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

}   // namespace

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: b_thin_host_check cases.txt\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    static SpdpScoring sc;
    memset(&sc, 0, sizeof sc);
    float tgapf = 1.f;
    bool have_sc = false;
    std::vector<uint8_t> a, b;
    char kind[2];
    while (fscanf(f, "%1s", kind) == 1) {
        if (kind[0] == 'S') {
            memset(&sc, 0, sizeof sc);
            sc.mtx_dim = rd(f);
            if (sc.mtx_dim < 1 || sc.mtx_dim > 32) { fprintf(stderr, "mtx_dim\n"); return 2; }
            for (int i = 0; i < sc.mtx_dim * sc.mtx_dim; ++i) sc.mtx[i] = rd(f);
            sc.gop = rd(f); sc.gep = rd(f); sc.lgop = rd(f); sc.lgep = rd(f); sc.codonk1 = rd(f); sc.noll = rd(f); sc.local = rd(f); sc.sh = rd(f);
            if (fscanf(f, "%f", &tgapf) != 1) return 2;
            sc.scalar_engines = 1;
            have_sc = true;
        } else if (kind[0] == 'P') {
            const int a_len = rd(f), b_len = rd(f);
            if (a_len < 0 || b_len < 0) return 2;
            a.assign((size_t) a_len, 0); b.assign((size_t) b_len, 0);
            for (int i = 0; i < a_len; ++i) a[i] = (uint8_t) rd(f);
            for (int i = 0; i < b_len; ++i) b[i] = (uint8_t) rd(f);
        } else if (kind[0] == 'C') {
            if (!have_sc) { fprintf(stderr, "a case before its bundle\n"); return 2; }
            SpdpProblem p;
            memset(&p, 0, sizeof p);
            const int id = rd(f);
            p.a = a.data(); p.a_len = (int) a.size(); p.b = b.data(); p.b_len = (int) b.size();
            p.a_left = rd(f); p.a_right = rd(f); p.b_left = rd(f); p.b_right = rd(f);
            p.a_exgl = (uint8_t) rd(f); p.a_exgr = (uint8_t) rd(f); p.b_exgl = (uint8_t) rd(f); p.b_exgr = (uint8_t) rd(f);
            const bool thin_allowed = rd(f) != 0;
            if (p.a_left < 0 || p.a_left > p.a_right || p.a_right > p.a_len || p.b_left < 0 || p.b_left > p.b_right || p.b_right > p.b_len) {
                fprintf(stderr, "case %d: a range outside its sequence\n", id); return 2;
            }
            SpdpWindow w;
            ladder::stripe<1>(p.a_left, p.a_right, p.b_left, p.b_right, sc.sh, &w);
            std::vector<SpdpSkl> rec;
            int served;
            bool failed;
            const int score = b_sweep_host::request(sc, tgapf, p, w, thin_allowed, rec, served, failed);
            if (failed) { printf("%d FAILED\n", id); continue; }
            printf("%d %d %d %d", id, score, served, (int) rec.size());
            for (const SpdpSkl& r : rec) printf(" %d %d", r.m, r.n);
            printf("\n");
        } else { fprintf(stderr, "unknown record %s\n", kind); return 2; }
    }
    fclose(f);
    return 0;
}
