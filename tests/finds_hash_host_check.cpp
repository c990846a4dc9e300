// finds_hash_host_check.cpp -- the finds vote's wave (spaln_amd/csrc/spdp_blk_finds.h, host flavour) with its scores in the
// open-addressed TABLE instead of the slab, and the host's part of that form around it: a query whose table ran full wrote nothing,
// and is run again on a table four times the size until it fits.  Reads the text dump of tests/finds_cases.py (dump_index /
// dump_query) as tests/finds_host_check.cpp does; built with -fsanitize=address,undefined and run by tests/test_finds_hash_host.py.
//     finds_hash_host_check <dump> <S> [any]
// S: the slots of the first table (a power of two).  One wave's state -- the tables of every size with their tags, the run hash's
// epochs, the heap's memory -- lives across the queries of an index, as on the device.  Per query one line:
//     <id> OK|FAILED <runs after a full table> <distinct blocks scored> <slots of the last table> [the record it got, when FAILED]
// any: the records are not compared (a malformed index: the run has to end, inside the table, and say nothing to the sanitizers).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "../spaln_amd/csrc/spdp_blk_finds.h"

namespace {

struct Index {
    BlkDev X;
    std::vector<uint8_t> convtab; std::vector<uint16_t> nblk; std::vector<int16_t> wscr;
    std::vector<int32_t> blkp, rscrtab, chr, bitpat, lenadj; std::vector<uint32_t> blkb;
    int max_out = 1, ptpl = 0, maxmmc = 0, hh_size = 31, hh_step = 8;
    // the wave: no slab -- a table per size, each of exactly 2 S words (a probe outside it is the sanitizer's to find)
    std::vector<int> st, as; std::vector<uint32_t> own, stage; std::vector<uint64_t> heap, hh;
    std::map<uint32_t, std::vector<uint64_t>> tables;
    uint32_t tag = 0;
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
    I.heap.assign((size_t) X.ncand + 1, 0); I.hh.assign((size_t) I.hh_size, 0);
    I.stage.assign(2 * (size_t) X.maxlist + 2, 0);
    FindsWave& W = I.W;
    W.X = &I.X; W.lenadj = I.lenadj.data(); W.n_words = (int64_t) n_words; W.max_out = I.max_out; W.ptpl = I.ptpl; W.maxmmc = I.maxmmc;
    W.st = I.st.data(); W.as = I.as.data(); W.own = I.own.data(); W.heap = I.heap.data();
    W.hh = I.hh.data(); W.hh_n = (uint32_t) I.hh_size; W.hh_step = (uint32_t) I.hh_step; W.epoch = 0;
    W.rscr = nullptr; W.tag = 0; W.stage = I.stage.data();
    W.store = 1;
}

void use_table(Index& I, uint32_t slots)
{
    std::vector<uint64_t>& t = I.tables[slots];
    if (t.empty()) t.assign(2 * (size_t) slots, 0);
    I.W.tb = t.data(); I.W.tb_n = slots; I.W.tb_shift = 32u - (uint32_t) __builtin_ctz(slots);
}

}   // namespace

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: finds_hash_host_check <dump> <S> [any]\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const uint32_t first = (uint32_t) strtoul(argv[2], nullptr, 10);
    if (first < 2 || (first & (first - 1))) { fprintf(stderr, "S: a power of two\n"); return 2; }
    const bool any = argc > 3 && !strcmp(argv[3], "any");
    Index* I = nullptr;
    std::string t;
    int failed = 0;
    while (next_token(f, t)) {
        if (t == "INDEX") { delete I; I = new Index; read_index(f, *I); continue; }
        if (t != "QUERY" || !I) { fprintf(stderr, "dump: unexpected %s\n", t.c_str()); return 2; }
        const int id = (int) next_int(f), left = (int) next_int(f), right = (int) next_int(f), out_cap = (int) next_int(f);
        std::vector<uint8_t> q; read_array(f, q, (size_t) next_int(f));
        std::vector<int32_t> want; read_array(f, want, (size_t) next_int(f));
        const int32_t untouched = -0x5a5a5a5a;
        std::vector<int32_t> out((size_t) out_cap, untouched);   // (exactly out_cap ints: a write past the record is the sanitizer's to find)
        // the largest table a query can need: nseg + 1 slots cannot fill
        uint32_t most = 64;
        while (most < (uint32_t) I->X.nseg + 1) most <<= 1;
        int again = 0;
        bool wrote_when_full = false;
        for (uint32_t slots = first; ; ) {
            use_table(*I, slots);
            I->W.tag = ++I->tag;
            if (!finds_query(I->W, q.data(), (int) q.size(), left, right, out.data(), out_cap)) break;
            for (int32_t v : out) wrote_when_full = wrote_when_full || v != untouched;
            if (slots >= most) { fprintf(stderr, "%d: a table of %u slots ran full with nseg = %d\n", id, slots, I->X.nseg); return 3; }
            ++again;
            slots = slots > most / 4 ? most : slots * 4;
        }
        for (int32_t& v : out) if (v == untouched) v = 0;         // (the caller's records start as zeros)
        const size_t n = out_cap > 0 ? (size_t) out[0] : 0;
        bool same = !wrote_when_full && n <= out.size();
        if (!any) same = same && n == want.size() && std::equal(want.begin(), want.end(), out.begin());
        printf("%d %s %d %d %u", id, same ? "OK" : "FAILED", again, I->W.n_scored, I->W.tb_n);
        if (!same) { ++failed; for (size_t i = 0; i < n && i < out.size(); ++i) printf(" %d", out[i]); }
        printf("\n");
    }
    delete I;
    fclose(f);
    return failed ? 1 : 0;
}
