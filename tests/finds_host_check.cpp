// finds_host_check.cpp -- the wave's logic of the finds vote (spaln_amd/csrc/spdp_blk_finds.h, host flavour: a per-lane value
// is an array of 64, a phase a loop) on a text dump of recipes: indexes, queries and the records the restatement wants.  Built with
// -fsanitize=address,undefined and run by tests/test_finds_host.py; one wave's state (slab tags, run-hash epochs, the heap's LDS)
// lives across the queries of an index, as on the device.  Prints "<id> OK" or "<id> FAILED <the record it got>" per query.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../spaln_amd/csrc/spdp_blk_finds.h"

namespace {

struct Index {
    BlkDev X;
    std::vector<uint8_t> convtab; std::vector<uint16_t> nblk; std::vector<int16_t> wscr;
    std::vector<int32_t> blkp, rscrtab, chr, bitpat, lenadj; std::vector<uint32_t> blkb;
    int max_out = 1, ptpl = 0, maxmmc = 0, hh_size = 31, hh_step = 8;
    // the wave
    std::vector<int> st, as; std::vector<uint32_t> own, stage; std::vector<uint64_t> heap, hh, rscr;
    FindsWave W;
};

bool next_token(FILE* f, std::string& t)
{
    char buf[64];
    if (fscanf(f, "%63s", buf) != 1) return false;
    t = buf;
    return true;
}
long long next_int(FILE* f) { long long v = 0; if (fscanf(f, "%lld", &v) != 1) { fprintf(stderr, "dump: integer expected\n"); exit(2); } return v; }
double next_real(FILE* f) { char buf[64]; if (fscanf(f, "%63s", buf) != 1) { fprintf(stderr, "dump: number expected\n"); exit(2); } return strtod(buf, nullptr); }
template <class T> void read_array(FILE* f, std::vector<T>& a, size_t n) { a.resize(n); for (size_t i = 0; i < n; ++i) a[i] = (T) next_int(f); }

void read_index(FILE* f, Index& I)
{
    BlkDev& X = I.X;
    memset(&X, 0, sizeof X);
    X.nalpha = (int) next_int(f); X.tabsize = (int) next_int(f); X.nshift = (int) next_int(f); X.nbitpat = (int) next_int(f);
    X.convts = (int) next_int(f); X.n_chr = (int) next_int(f); X.kk = (int) next_int(f); X.nseg = (int) next_int(f);
    X.ncand = (int) next_int(f); X.maxlist = (int) next_int(f); I.hh_size = (int) next_int(f); I.hh_step = (int) next_int(f);
    X.gdb = (int) next_int(f); I.max_out = (int) next_int(f); I.ptpl = (int) next_int(f); I.maxmmc = (int) next_int(f);
    const size_t n_words = (size_t) next_int(f), n_bitpat = (size_t) next_int(f);
    X.rbscoef = (float) next_real(f); X.rbscons = (float) next_real(f);
    X.bclw = next_real(f); X.bcup = next_real(f); X.bcce = next_real(f); X.app_c = next_real(f);
    read_array(f, I.convtab, (size_t) X.convts); read_array(f, I.nblk, (size_t) X.tabsize); read_array(f, I.wscr, (size_t) X.tabsize);
    read_array(f, I.blkp, (size_t) X.tabsize); read_array(f, I.blkb, n_words); read_array(f, I.rscrtab, 128);
    read_array(f, I.chr, 2 * ((size_t) X.n_chr + 1)); read_array(f, I.bitpat, n_bitpat); read_array(f, I.lenadj, (size_t) X.nseg + 1);
    X.convtab = I.convtab.data(); X.nblk = I.nblk.data(); X.wscr = I.wscr.data(); X.blkp = I.blkp.data(); X.blkb = I.blkb.data();
    X.rscrtab = I.rscrtab.data(); X.chr = I.chr.data(); X.bitpat = I.bitpat.data();
    int at = 0;
    for (int k = 0; k < X.kk; ++k) { X.pat_off[k] = at; at += 3 + 2 * I.bitpat[(size_t) at]; }
    I.st.assign(FST_WORDS, 0); I.as.assign(64, 0); I.own.assign(SPDP_FINDS_OWN, 0xffffffffu);
    I.heap.assign((size_t) X.ncand + 1, 0); I.hh.assign((size_t) I.hh_size, 0); I.rscr.assign((size_t) X.nseg + 1, 0);
    I.stage.assign(2 * (size_t) X.maxlist + 2, 0);
    FindsWave& W = I.W;
    W.X = &I.X; W.lenadj = I.lenadj.data(); W.n_words = (int64_t) n_words; W.max_out = I.max_out; W.ptpl = I.ptpl; W.maxmmc = I.maxmmc;
    W.st = I.st.data(); W.as = I.as.data(); W.own = I.own.data(); W.heap = I.heap.data();
    W.hh = I.hh.data(); W.hh_n = (uint32_t) I.hh_size; W.hh_step = (uint32_t) I.hh_step; W.epoch = 0;
    W.rscr = I.rscr.data(); W.tag = 0; W.stage = I.stage.data();
}

}   // namespace

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: finds_host_check <dump>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    Index* I = nullptr;
    std::string t;
    int failed = 0;
    while (next_token(f, t)) {
        if (t == "INDEX") { delete I; I = new Index; read_index(f, *I); continue; }
        if (t != "QUERY" || !I) { fprintf(stderr, "dump: unexpected %s\n", t.c_str()); return 2; }
        const int id = (int) next_int(f), left = (int) next_int(f), right = (int) next_int(f), out_cap = (int) next_int(f);
        std::vector<uint8_t> q; read_array(f, q, (size_t) next_int(f));
        std::vector<int32_t> want; read_array(f, want, (size_t) next_int(f));
        std::vector<int32_t> out((size_t) out_cap, 0);          // (exactly out_cap ints: a write past the record is the sanitizer's to find)
        ++I->W.tag;
        finds_query(I->W, q.data(), (int) q.size(), left, right, out.data(), out_cap);
        const size_t n = out_cap > 0 ? (size_t) out[0] : 0;
        const bool same = n == want.size() && n <= out.size() && std::equal(want.begin(), want.end(), out.begin());
        printf("%d %s", id, same ? "OK" : "FAILED");
        if (!same) { ++failed; for (size_t i = 0; i < n && i < out.size(); ++i) printf(" %d", out[i]); }
        printf("\n");
    }
    delete I;
    fclose(f);
    return failed ? 1 : 0;
}
