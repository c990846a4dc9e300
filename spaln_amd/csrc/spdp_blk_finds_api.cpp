// spdp_blk_finds_api.cpp -- host side of the finds vote (include/spdp.h, "protein database search"): what the kernel needs beside
// the resident index (the length corrections of the blocks, the waves' areas) is made on the first call and kept with the index;
// a call uploads its queries, runs spdp_blk_finds_wave (a wave per query, waves persistent) and brings the records back.  What
// holds the scores -- the slab or the table -- is chosen when the index is first searched (spdp_blk_finds_dev.h); in the table
// form the queries whose table ran full are run again here, on larger tables, until none is left.
#include "spdp_internal.h"
#include "spdp_blk_dev.h"
#include "spdp_blk_finds_dev.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

struct Kept : BlkFindsKept {
    int32_t* d_lenadj = nullptr; float rln_coef = -1.f;
    uint8_t* slabs = nullptr; uint32_t* next = nullptr;
    size_t slab_bytes = 0; int n_waves = 0, hh_in_lds = 0; uint32_t lds_bytes = 0;
    int form = -1; uint32_t tb_n = 0;           // what holds the scores: 0 the slab, 1 the table of tb_n slots a wave
    // the table form's second set of areas, for the queries that are run again: more_waves tables of more_n slots
    uint8_t* more = nullptr; size_t more_bytes = 0; int more_waves = 0; uint32_t more_n = 0;
    int32_t* lists[2] = {nullptr, nullptr}; int list_cap = 0;   // a launch's overflow list and the list it ran
    ~Kept() override
    {
        if (d_lenadj) (void) hipFree(d_lenadj);
        if (slabs) (void) hipFree(slabs);
        if (more) (void) hipFree(more);
        if (next) (void) hipFree(next);
        for (int32_t* l : lists) if (l) (void) hipFree(l);
    }
};

// SPDP_FINDS_RSCR as the index's first search reads it: 0 the slab, 1 the table, -1 neither word
int form_asked(const BlkDev* v)
{
    const char* e = getenv("SPDP_FINDS_RSCR");
    if (!e || !*e) return v->nseg - 1 > SPDP_FINDS_MAX_BLOCKS ? 1 : 0;
    return !strcmp(e, "slab") ? 0 : !strcmp(e, "hash") ? 1 : -1;
}
uint32_t pow2_at_least(uint64_t x) { uint32_t p = SPDP_FINDS_TABLE_MIN_SLOTS; while (p < x && p < (1u << 31)) p <<= 1; return p; }
int waves_wanted(const SpdpContext* ctx, const Kept* K, size_t area_bytes, int n)
{
    const int per_cu = (int) std::max<size_t>(1, std::min<size_t>(16, ((size_t) 160 << 10) / std::max<uint32_t>(K->lds_bytes, 1)));
    size_t want = (size_t) std::max(1, ctx->n_cu) * per_cu;
    want = std::min(want, std::max<size_t>(1, SPDP_FINDS_SLAB_BUDGET / area_bytes));
    return (int) std::min<size_t>(want, (size_t) std::max(1, n));
}

// setSegLen (src/blksrc.cc:1966-1983) and Randbs::lencor (src/blksrc.h:460) of every block
int length_corrections(SpdpContext* ctx, Kept* K, const SpdpBlkIndexDesc* hix, float rln_coef)
{
    if (K->d_lenadj && K->rln_coef == rln_coef) return 0;
    std::vector<int32_t> adj((size_t) hix->nseg + 1, 0);
    int64_t blk = 0;
    for (int c = 0; c < hix->n_chr; ++c) {
        int64_t len = (int64_t) (uint32_t) hix->chr[2 * (c + 1)] - (int64_t) (uint32_t) hix->chr[2 * c];
        for ( ; len > 0; len -= hix->blklen) {
            if (++blk >= hix->nseg) { ctx->err = "spdp_blk_finds: the sequences of the index hold more blocks than nseg (SrchBlk::setSegLen block # mismatch)"; return -1; }
            adj[blk] = (int32_t) (rln_coef * sqrt((double) std::min<int64_t>(len, hix->blklen)));
        }
    }
    if (!K->d_lenadj) HIPCHK(hipMalloc((void**) &K->d_lenadj, adj.size() * 4));
    HIPCHK(hipMemcpy(K->d_lenadj, adj.data(), adj.size() * 4, hipMemcpyHostToDevice));
    K->rln_coef = rln_coef;
    return 0;
}

int ensure_waves(SpdpContext* ctx, Kept* K, const BlkDev* v, int n)
{
    if (!K->slab_bytes) {
        K->hh_in_lds = (size_t) v->hh_size1 * 8 <= SPDP_FINDS_HH_LDS_BYTES;
        if (const char* e = getenv("SPDP_FINDS_HH_LDS")) K->hh_in_lds = K->hh_in_lds && atoi(e) != 0;
        K->form = form_asked(v);
        if (K->form) {
            const char* e = getenv("SPDP_FINDS_RSCR_SLOTS");
            const long long asked = e ? atoll(e) : 0;
            K->tb_n = asked > 0 ? pow2_at_least((uint64_t) asked) : SPDP_FINDS_TABLE_SLOTS;
        }
        K->lds_bytes = spdp_blk_finds_lds_bytes(v, v->hh_size1, K->hh_in_lds);
        K->slab_bytes = spdp_blk_finds_area_bytes(v, v->hh_size1, K->hh_in_lds, K->tb_n);
    }
    if (K->lds_bytes > (64u << 10)) { ctx->err = "spdp_blk_finds: the heap of a query does not fit the LDS of a workgroup (ncand too large)"; return -1; }
    const int want = waves_wanted(ctx, K, K->slab_bytes, n);   // (the slab: the budget may set it; the table: the CU count does)
    if (!K->next) HIPCHK(hipMalloc((void**) &K->next, 16));
    if (K->form && n > K->list_cap) {
        for (int32_t*& l : K->lists) { if (l) (void) hipFree(l); l = nullptr; }
        K->list_cap = 0;
        for (int32_t*& l : K->lists) HIPCHK(hipMalloc((void**) &l, (size_t) n * 4));
        K->list_cap = n;
    }
    if (want <= K->n_waves) return 0;
    if (K->slabs) { (void) hipFree(K->slabs); K->slabs = nullptr; }
    K->n_waves = 0;
    HIPCHK(hipMalloc((void**) &K->slabs, (size_t) want * K->slab_bytes));
    HIPCHK(hipMemsetAsync(K->slabs, 0, (size_t) want * K->slab_bytes, ctx->stream));    // (tags and epochs of no query: every slot reads as empty)
    K->n_waves = want;
    return 0;
}

// areas with tables of tb_n slots for n queries that are run again; fewer waves when the device has no room for as many
int ensure_more(SpdpContext* ctx, Kept* K, const BlkDev* v, uint32_t tb_n, int n)
{
    const size_t bytes = spdp_blk_finds_area_bytes(v, v->hh_size1, K->hh_in_lds, tb_n);
    int want = waves_wanted(ctx, K, bytes, n);
    if (K->more && K->more_n == tb_n && K->more_waves >= want) return 0;
    if (K->more) { (void) hipFree(K->more); K->more = nullptr; }
    K->more_waves = 0;
    for ( ; ; want = (want + 1) / 2) {
        if (hipMalloc((void**) &K->more, (size_t) want * bytes) == hipSuccess) break;
        (void) hipGetLastError();
        K->more = nullptr;
        if (want == 1) { ctx->err = "spdp_blk_finds: no device memory for one wave's score table (a query scored more blocks than the table before held; SPDP_FINDS_RSCR, DESIGN.md 5b)"; return -1; }
    }
    HIPCHK(hipMemsetAsync(K->more, 0, (size_t) want * bytes, ctx->stream));
    K->more_bytes = bytes; K->more_n = tb_n; K->more_waves = want;
    return 0;
}

// what both entries refuse before they touch the device
const char* refusal(const SpdpContext* ctx, const SpdpBlkIndex* ix, const SpdpBlkIndexDesc* hix, const SpdpBlkFindsParams* prm, int out_cap)
{
    if (!ix || !hix || !prm) return "spdp_blk_finds: null argument";
    if (spdp_blk_index_ctx(ix) != ctx) return "spdp_blk_finds: the index belongs to another context";
    const BlkDev* v = spdp_blk_index_view(ix);
    if (v->drna || hix->drna) return "spdp_blk_finds: a nucleotide index (protein queries search the amino-acid index of a protein database, spaln -W -KA)";
    if (v->gdb || hix->gdb) return "spdp_blk_finds: the index was read for a genomic database (SpdpBlkSearchOpts.genomic_db = 0 selects Randbs' form for finds)";
    if (hix->nseg != v->nseg || hix->n_chr != v->n_chr || !hix->chr || hix->blklen < 1 || hix->n_words != spdp_blk_index_n_words(ix)) return "spdp_blk_finds: the host description is not the resident index's";
    if (prm->max_out < 1 || v->ncand != prm->max_out + 10) return "spdp_blk_finds: the index was not made for max_out (Ncand != MaxOut + 10, src/blksrc.cc:2220)";
    const BlkFindsKept* kept = spdp_blk_index_finds_kept(const_cast<SpdpBlkIndex*>(ix));
    const int form = kept && static_cast<const Kept*>(kept)->form >= 0 ? static_cast<const Kept*>(kept)->form : form_asked(v);
    if (form < 0) return "spdp_blk_finds: SPDP_FINDS_RSCR is neither slab nor hash";
    if (!form && v->nseg - 1 > SPDP_FINDS_MAX_BLOCKS) return "spdp_blk_finds: a database of more than 2^24 blocks (the score slab of a wave holds 8 bytes a block)";
    if (prm->ptpl < 0 || !(prm->rln_coef >= 0.f)) return "spdp_blk_finds: ptpl / rln_coef out of range";
    if (out_cap < 6) return "spdp_blk_finds: out_cap < 6";
    return nullptr;
}

}   // namespace

extern "C" int spdp_blk_finds_resident(SpdpContext* ctx, const SpdpBlkIndex* cix, const SpdpBlkIndexDesc* hix, const SpdpBlkFindsParams* prm,
                                       const uint8_t* d_codes, const int64_t* d_offs, const int32_t* d_left, const int32_t* d_right, int32_t n,
                                       int32_t* d_out, int32_t out_cap, float* kernel_ms)
{
    if (!ctx) return -1;
    if (const char* why = refusal(ctx, cix, hix, prm, out_cap)) { ctx->err = why; return -1; }
    if (n <= 0) return 0;
    if (!d_codes || !d_offs || !d_left || !d_right || !d_out) { ctx->err = "spdp_blk_finds: null argument"; return -1; }
    SpdpBlkIndex* ix = const_cast<SpdpBlkIndex*>(cix);
    (void) hipSetDevice(ctx->device);
    BlkFindsKept*& slot = spdp_blk_index_finds_kept(ix);
    if (!slot) slot = new Kept;
    Kept* K = static_cast<Kept*>(slot);
    const BlkDev* v = spdp_blk_index_view(ix);
    if (length_corrections(ctx, K, hix, prm->rln_coef) || ensure_waves(ctx, K, v, n)) return -1;
    BlkFindsArgs A;
    memset(&A, 0, sizeof A);
    A.ix = spdp_blk_index_on_device(ix);
    if (!A.ix) return -1;
    A.lenadj = K->d_lenadj; A.n_words = hix->n_words; A.max_out = prm->max_out; A.ptpl = prm->ptpl;
    A.maxmmc = prm->local ? INT_MAX : v->maxmmc;
    A.codes = d_codes; A.offs = d_offs; A.left = d_left; A.right = d_right; A.out = d_out; A.out_cap = out_cap; A.n = n;
    A.slabs = K->slabs; A.slab_bytes = K->slab_bytes; A.next = K->next; A.n_waves = std::min(K->n_waves, n);
    A.hh_n = v->hh_size1; A.hh_step = v->hh_size2; A.hh_in_lds = K->hh_in_lds; A.lds_bytes = K->lds_bytes;
    A.tb_n = K->tb_n; A.which = nullptr; A.over = K->lists[0];
    int64_t* st = ctx->finds_store;
    memset(st, 0, sizeof ctx->finds_store);
    st[0] = K->form; st[1] = A.n_waves; st[2] = (int64_t) K->slab_bytes; st[3] = st[4] = K->tb_n;
    float ms_all = 0.f;
    // the table form: a launch, then the queries whose table ran full again on tables four times the size, until none is listed
    // (a table of nseg + 1 slots cannot fill: the loop ends)
    const uint32_t tb_most = pow2_at_least((uint64_t) v->nseg + 1);
    for (int round = 0; ; ++round) {
        HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
        HIPCHK(spdp_blk_finds_launch(&A, ctx->stream));
        HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        ms_all += ms; ++st[5];
        if (!K->form) break;
        uint32_t told[2] = {0, 0};                      // the launch's overflow count and the most blocks a query scored
        HIPCHK(hipMemcpy(told, K->next + 1, 8, hipMemcpyDeviceToHost));
        st[7] = std::max<int64_t>(st[7], told[1]);
        if (!told[0]) break;
        if (told[0] > (uint32_t) A.n || A.tb_n >= tb_most) { ctx->err = "spdp_blk_finds: the overflow list of a launch is not what a launch can write"; return -1; }
        const uint32_t grown = A.tb_n > tb_most / 4 ? tb_most : A.tb_n * 4;
        if (ensure_more(ctx, K, v, grown, (int) told[0])) return -1;
        st[6] += told[0]; st[4] = grown;
        A.which = A.over; A.over = K->lists[(round + 1) & 1]; A.n = (int) told[0];
        A.tb_n = grown; A.slabs = K->more; A.slab_bytes = K->more_bytes; A.n_waves = std::min(K->more_waves, A.n);
    }
    if (kernel_ms) *kernel_ms = ms_all;
    return 0;
}

extern "C" int spdp_blk_finds_store_stats(const SpdpContext* ctx, int64_t* out, int n)
{
    if (!ctx || !out) return -1;
    for (int i = 0; i < n && i < 8; ++i) out[i] = ctx->finds_store[i];
    return 0;
}

extern "C" int spdp_blk_finds(SpdpContext* ctx, const SpdpBlkIndex* ix, const SpdpBlkIndexDesc* hix, const SpdpBlkFindsParams* prm,
                              const uint8_t* codes, const int64_t* offs, const int32_t* left, const int32_t* right, int32_t n,
                              int32_t* out, int32_t out_cap, float* kernel_ms)
{
    if (!ctx) return -1;
    if (const char* why = refusal(ctx, ix, hix, prm, out_cap)) { ctx->err = why; return -1; }
    if (n <= 0) return 0;
    if (!codes || !offs || !left || !right || !out) { ctx->err = "spdp_blk_finds: null argument"; return -1; }
    for (int i = 0; i < n; ++i) {
        const int64_t len = offs[i + 1] - offs[i];
        if (len < 0 || len > INT32_MAX || left[i] < 0 || right[i] > len || right[i] < left[i]) { ctx->err = "spdp_blk_finds: bad query range"; return -1; }
    }
    (void) hipSetDevice(ctx->device);
    struct Dev { void* p = nullptr; ~Dev() { if (p) (void) hipFree(p); } } d_codes, d_offs, d_l, d_r, d_out;
    const size_t nb = (size_t) (offs[n] - offs[0]);
    HIPCHK(hipMalloc(&d_codes.p, std::max<size_t>(nb, 16)));
    HIPCHK(hipMalloc(&d_offs.p, ((size_t) n + 1) * 8));
    HIPCHK(hipMalloc(&d_l.p, (size_t) n * 4)); HIPCHK(hipMalloc(&d_r.p, (size_t) n * 4));
    HIPCHK(hipMalloc(&d_out.p, (size_t) n * out_cap * 4));
    std::vector<int64_t> rel((size_t) n + 1);
    for (int i = 0; i <= n; ++i) rel[i] = offs[i] - offs[0];
    HIPCHK(hipMemcpyAsync(d_codes.p, codes + offs[0], nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_offs.p, rel.data(), ((size_t) n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_l.p, left, (size_t) n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_r.p, right, (size_t) n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(d_out.p, 0, (size_t) n * out_cap * 4, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));          // (rel is a local: the copies must have read it)
    if (spdp_blk_finds_resident(ctx, ix, hix, prm, (const uint8_t*) d_codes.p, (const int64_t*) d_offs.p, (const int32_t*) d_l.p,
                                (const int32_t*) d_r.p, n, (int32_t*) d_out.p, out_cap, kernel_ms)) return -1;
    HIPCHK(hipMemcpy(out, d_out.p, (size_t) n * out_cap * 4, hipMemcpyDeviceToHost));
    return 0;
}
