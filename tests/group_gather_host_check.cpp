// group_gather_host_check.cpp -- spaln_amd/csrc/spdp_group_gather.h driven on shards a test describes (tests/test_group_gather_host.py).
// A program of its own, built with -fsanitize=address,undefined: no HIP, no library, nothing loaded into Python.
//
// Input (text):  CASE <members> <n>            then for each of the n queries, in the caller's order:
//                Q <member> <records>          who serves it (-1: nobody) and how long its list is
//                R <value> <k> <s0> .. <sk-1>  one line per record: its value and the entries of its side array
// Every member's answer is laid out as a single-context entry would write it for that shard -- its queries numbered from 0, its
// lists pooled, its side entries pooled with offsets of its own (behind one unused entry, so that an offset that is merely copied
// shows) -- and gathered in the three shapes.  Output per case:
//   V  two values per query (its record count, the sum of its values), scattered        P <r> ..  what pick() hands member r of V's source
//   T  totals: records, side entries                                                    O  the list offsets, n + 1
//   L  the records' values   K  their query numbers   S  their side offsets   D  the side array
//   M  O and L again through the form without a side array
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../spaln_amd/csrc/spdp_group_gather.h"

struct Rec { int32_t query; int32_t value; int32_t n_side; int64_t side_off; };
struct Side { int32_t a, b; };

struct Query { int member; std::vector<Rec> rec; std::vector<std::vector<int32_t>> side; };

static void line(const char* tag, const std::vector<long long>& v)
{
    printf("%s", tag);
    for (long long x : v) printf(" %lld", x);
    printf("\n");
}

static int run_case(int w, const std::vector<Query>& q)
{
    using namespace spdp_gather;
    const int n = (int) q.size();
    std::vector<std::vector<int>> idx((size_t) w);
    for (int i = 0; i < n; ++i) if (q[i].member >= 0) idx[(size_t) q[i].member].push_back(i);
    // ---- the members' answers
    std::vector<Part<Rec, Side>> got((size_t) w);
    std::vector<Part<int32_t>> plain((size_t) w);
    std::vector<int32_t> source((size_t) 2 * n), scattered((size_t) 2 * n, -7);
    for (int i = 0; i < n; ++i) {
        long long sum = 0;
        for (const Rec& r : q[i].rec) sum += r.value;
        source[2 * i] = (int32_t) q[i].rec.size(); source[2 * i + 1] = (int32_t) sum;
    }
    for (int r = 0; r < w; ++r) {
        if (idx[r].empty()) continue;                                   // (a member without queries is never called)
        Part<Rec, Side>& P = got[r];
        const int cnt = (int) idx[r].size();
        std::vector<int64_t> off((size_t) cnt + 1, 0);
        P.side.push_back({-1, -1});
        for (int k = 0; k < cnt; ++k) {
            const Query& Q = q[(size_t) idx[r][k]];
            for (size_t j = 0; j < Q.rec.size(); ++j) {
                Rec x = Q.rec[j];
                x.query = k; x.n_side = (int32_t) Q.side[j].size(); x.side_off = (int64_t) P.side.size();
                for (int32_t s : Q.side[j]) P.side.push_back({s, -s});
                P.rec.push_back(x);
            }
            off[(size_t) k + 1] = (int64_t) P.rec.size();
        }
        P.off = offsets_by_query(P.rec.data(), (int64_t) P.rec.size(), cnt, &Rec::query);
        if (P.off != off) { printf("FAILED offsets_by_query member %d\n", r); return 1; }
        const size_t used = side_extent(P.rec.data(), (int64_t) P.rec.size(), &Rec::side_off, [](const Rec& x) { return x.n_side; });
        bool any = false;
        for (const Rec& x : P.rec) any = any || x.n_side > 0;
        if (used != (any ? P.side.size() : 0)) {
            // (side entries are appended in record order: the last record with entries ends the pool)
            printf("FAILED side_extent member %d: %zu of %zu\n", r, used, P.side.size()); return 1;
        }
        P.side.resize(used);                                            // what a caller of a malloc'ed pool can know of it
        plain[r].off = P.off;
        for (const Rec& x : P.rec) plain[r].rec.push_back(x.value);
        // shape 1
        const std::vector<int32_t> mine = pick(idx[r], (const int32_t*) source.data(), 2);
        std::vector<long long> pv(1, r);
        pv.insert(pv.end(), mine.begin(), mine.end());
        line("P", pv);
        scatter(idx[r], mine.data(), scattered.data(), 2);
        if (!pick(idx[r], (const int32_t*) nullptr, 2).empty()) { printf("FAILED pick of nothing\n"); return 1; }
        scatter(idx[r], mine.data(), (int32_t*) nullptr, 2);
    }
    line("V", std::vector<long long>(scattered.begin(), scattered.end()));
    // ---- shapes 2 and 3
    const std::vector<Place> at = places(n, idx);
    const auto count = [](const Rec& x) { return x.n_side; };
    const Totals t = totals(at, got, count);
    const Totals t2 = totals(at, plain);
    if (t2.rec != t.rec || t2.side != 0) { printf("FAILED totals without a side array\n"); return 1; }
    line("T", {(long long) t.rec, (long long) t.side});
    // exactly as large as totals() says: a write past either pool is the sanitizer's to report
    Rec* rec = (Rec*) malloc(sizeof(Rec) * (t.rec ? t.rec : 1));
    Side* side = (Side*) malloc(sizeof(Side) * (t.side ? t.side : 1));
    int32_t* vals = (int32_t*) malloc(sizeof(int32_t) * (t.rec ? t.rec : 1));
    std::vector<int64_t> off((size_t) n + 1, -1), off2((size_t) n + 1, -1);
    gather_lists(at, got, off.data(), rec, side, &Rec::side_off, count, [](Rec& x, int caller) { x.query = caller; });
    gather_lists(at, plain, off2.data(), vals);
    line("O", std::vector<long long>(off.begin(), off.end()));
    std::vector<long long> L, K, S, D, M(off2.begin(), off2.end());
    for (size_t k = 0; k < t.rec; ++k) { L.push_back(rec[k].value); K.push_back(rec[k].query); S.push_back(rec[k].side_off); M.push_back(vals[k]); }
    for (size_t k = 0; k < t.side; ++k) { D.push_back(side[k].a); if (side[k].b != -side[k].a) { printf("FAILED side entry %zu\n", k); return 1; } }
    line("L", L); line("K", K); line("S", S); line("D", D); line("M", M);
    // the form the locus search uses: no offsets out, the records say whose they are
    Rec* rec2 = (Rec*) malloc(sizeof(Rec) * (t.rec ? t.rec : 1));
    gather_lists(at, got, (int64_t*) nullptr, rec2, side, &Rec::side_off, count, [](Rec& x, int caller) { x.query = caller; });
    if (t.rec && memcmp(rec, rec2, sizeof(Rec) * t.rec)) { printf("FAILED without offsets\n"); return 1; }
    free(rec); free(rec2); free(side); free(vals);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: group_gather_host_check cases.txt\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    char tag[8];
    int w = 0, n = 0;
    while (fscanf(f, "%7s", tag) == 1) {
        if (strcmp(tag, "CASE")) { fprintf(stderr, "expected CASE\n"); return 2; }
        if (fscanf(f, "%d %d", &w, &n) != 2 || w < 1 || n < 0) return 2;
        std::vector<Query> q((size_t) n);
        for (int i = 0; i < n; ++i) {
            int nrec = 0;
            if (fscanf(f, "%7s %d %d", tag, &q[i].member, &nrec) != 3 || strcmp(tag, "Q") || q[i].member >= w || nrec < 0) return 2;
            for (int j = 0; j < nrec; ++j) {
                int v = 0, k = 0;
                if (fscanf(f, "%7s %d %d", tag, &v, &k) != 3 || strcmp(tag, "R") || k < 0) return 2;
                Rec r;
                memset(&r, 0, sizeof r);
                r.value = v;
                std::vector<int32_t> s((size_t) k);
                for (int x = 0; x < k; ++x) if (fscanf(f, "%d", &s[x]) != 1) return 2;
                q[i].rec.push_back(r); q[i].side.push_back(s);
            }
        }
        printf("CASE %d %d\n", w, n);
        if (run_case(w, q)) return 1;
    }
    fclose(f);
    return 0;
}
