// spdp_blk_finds_api.cpp -- host side of the finds vote (include/spdp.h, "protein database search"): what the kernel needs beside
// the resident index (the length corrections of the blocks, the waves' slabs) is made on the first call and kept with the index;
// a call uploads its queries, runs spdp_blk_finds_wave (a wave per query, waves persistent) and brings the records back.
#include "spdp_internal.h"
#include "spdp_blk_dev.h"
#include "spdp_blk_finds_dev.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

struct Kept : BlkFindsKept {
    int32_t* d_lenadj = nullptr; float rln_coef = -1.f;
    uint8_t* slabs = nullptr; uint32_t* next = nullptr;
    size_t slab_bytes = 0; int n_waves = 0, hh_in_lds = 0; uint32_t lds_bytes = 0;
    ~Kept() override
    {
        if (d_lenadj) (void) hipFree(d_lenadj);
        if (slabs) (void) hipFree(slabs);
        if (next) (void) hipFree(next);
    }
};

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
        K->lds_bytes = spdp_blk_finds_lds_bytes(v, v->hh_size1, K->hh_in_lds);
        K->slab_bytes = spdp_blk_finds_slab_bytes(v, v->hh_size1, K->hh_in_lds);
    }
    if (K->lds_bytes > (64u << 10)) { ctx->err = "spdp_blk_finds: the heap of a query does not fit the LDS of a workgroup (ncand too large)"; return -1; }
    const int per_cu = (int) std::max<size_t>(1, std::min<size_t>(16, ((size_t) 160 << 10) / std::max<uint32_t>(K->lds_bytes, 1)));
    size_t want = (size_t) std::max(1, ctx->n_cu) * per_cu;
    want = std::min(want, std::max<size_t>(1, SPDP_FINDS_SLAB_BUDGET / K->slab_bytes));
    want = std::min<size_t>(want, (size_t) std::max(1, n));
    if (!K->next) HIPCHK(hipMalloc((void**) &K->next, 16));
    if ((int) want <= K->n_waves) return 0;
    if (K->slabs) { (void) hipFree(K->slabs); K->slabs = nullptr; }
    K->n_waves = 0;
    HIPCHK(hipMalloc((void**) &K->slabs, want * K->slab_bytes));
    HIPCHK(hipMemsetAsync(K->slabs, 0, want * K->slab_bytes, ctx->stream));    // (tags and epochs of no query: every slot reads as empty)
    K->n_waves = (int) want;
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
    if (v->nseg - 1 > SPDP_FINDS_MAX_BLOCKS) return "spdp_blk_finds: a database of more than 2^24 blocks (the score slab of a wave holds 8 bytes a block)";
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
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    HIPCHK(spdp_blk_finds_launch(&A, ctx->stream));
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (kernel_ms) HIPCHK(hipEventElapsedTime(kernel_ms, ctx->ev0, ctx->ev1));
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
