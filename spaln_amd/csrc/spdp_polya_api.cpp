// spdp_polya_api.cpp -- the entries of the query preparation (include/spdp.h "query preparation"): the sequential rule on the
// host (spdp_polya_scan_host: the record the device form is held to), and the device form on queries the caller uploads
// (spdp_polya_scan) or has resident already (spdp_polya_scan_resident).  spdp_map_align_s_prep runs the resident form on the
// queries before the block search (spdp_map_api.cpp).
#include "spdp_internal.h"
#include "spdp_polya.h"
#include <algorithm>
#include <cstring>
#include <vector>

// what a preparation may ask for; null: fine, otherwise the reason it is refused
const char* spdp_prep_refused(const SpdpQueryPrep* prep)
{
    if (!prep) return "null SpdpQueryPrep";
    if (prep->q_mns == 2) return "q_mns = 2 (the complementary strand alone, -S2) is not served";
    if (prep->q_mns != 1 && prep->q_mns != 3) return "q_mns must be 1 (-S1) or 3 (both orientations, the program's default)";
    return nullptr;
}

extern "C" int spdp_polya_scan_host(const uint8_t* codes, const int64_t* offs, int32_t n, const SpdpQueryPrep* prep,
                                    SpdpQueryTail* tails, uint8_t* codes_out)
{
    if (spdp_prep_refused(prep)) return -1;
    if (n <= 0) return 0;
    if (!codes || !offs || !tails) return -1;
    for (int i = 0; i < n; ++i) if (offs[i + 1] < offs[i] || offs[i + 1] - offs[i] > INT32_MAX) return -1;
    for (int i = 0; i < n; ++i) {
        const uint8_t* q = codes + offs[i];
        const int32_t len = (int32_t) (offs[i + 1] - offs[i]);
        const bool turn = spdp_polya::decide(q, len, prep->q_mns, prep->polya_thr, tails + i);
        if (!codes_out) continue;
        uint8_t* o = codes_out + offs[i];
        if (!turn) { if (o != q) memmove(o, q, (size_t) len); continue; }
        for (int32_t l = 0, r = len - 1; l <= r; ++l, --r) {       // (in place when the caller passes codes_out = codes)
            const uint8_t x = q[l], y = q[r];
            o[l] = spdp_polya::other_strand(y); o[r] = spdp_polya::other_strand(x);
        }
    }
    return 0;
}

extern "C" int spdp_polya_scan_resident(SpdpContext* ctx, uint8_t* d_codes, const int64_t* d_offs, int32_t n, const SpdpQueryPrep* prep,
                                        SpdpQueryTail* d_tails, float* kernel_ms)
{
    if (!ctx) return -1;
    if (const char* why = spdp_prep_refused(prep)) { ctx->err = std::string("spdp_polya_scan: ") + why; return -1; }
    if (kernel_ms) *kernel_ms = 0;
    if (n <= 0) return 0;
    if (!d_codes || !d_offs || !d_tails) { ctx->err = "spdp_polya_scan: null argument"; return -1; }
    (void) hipSetDevice(ctx->device);
    const PolyaArgs A = {d_codes, d_offs, n, prep->q_mns, prep->polya_thr, d_tails};
    if (kernel_ms) HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    HIPCHK(spdp_polya_launch(&A, ctx->stream));
    if (kernel_ms) {                                    // (a caller that does not ask for the time is not made to wait: the stream orders what follows)
        HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        HIPCHK(hipEventElapsedTime(kernel_ms, ctx->ev0, ctx->ev1));
    }
    return 0;
}

extern "C" int spdp_polya_scan(SpdpContext* ctx, const uint8_t* codes, const int64_t* offs, int32_t n, const SpdpQueryPrep* prep,
                               SpdpQueryTail* tails, uint8_t* codes_out, float* kernel_ms)
{
    if (!ctx) return -1;
    if (const char* why = spdp_prep_refused(prep)) { ctx->err = std::string("spdp_polya_scan: ") + why; return -1; }
    if (kernel_ms) *kernel_ms = 0;
    if (n <= 0) return 0;
    if (!codes || !offs || !tails) { ctx->err = "spdp_polya_scan: null argument"; return -1; }
    for (int i = 0; i < n; ++i)
        if (offs[i + 1] < offs[i] || offs[i + 1] - offs[i] > INT32_MAX) { ctx->err = "spdp_polya_scan: bad query offsets"; return -1; }
    (void) hipSetDevice(ctx->device);
    struct Dev { void* p = nullptr; ~Dev() { if (p) (void) hipFree(p); } } d_codes, d_offs, d_tails;
    const size_t nb = (size_t) (offs[n] - offs[0]);
    HIPCHK(hipMalloc(&d_codes.p, std::max<size_t>(nb, 16)));
    HIPCHK(hipMalloc(&d_offs.p, ((size_t) n + 1) * 8));
    HIPCHK(hipMalloc(&d_tails.p, (size_t) n * sizeof(SpdpQueryTail)));
    std::vector<int64_t> rel(n + 1);
    for (int i = 0; i <= n; ++i) rel[i] = offs[i] - offs[0];
    HIPCHK(hipMemcpyAsync(d_codes.p, codes + offs[0], nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_offs.p, rel.data(), ((size_t) n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));          // (rel is a local: the copy must have read it)
    float ms = 0;
    if (spdp_polya_scan_resident(ctx, (uint8_t*) d_codes.p, (const int64_t*) d_offs.p, n, prep, (SpdpQueryTail*) d_tails.p, &ms)) return -1;
    if (kernel_ms) *kernel_ms = ms;
    HIPCHK(hipMemcpy(tails, d_tails.p, (size_t) n * sizeof(SpdpQueryTail), hipMemcpyDeviceToHost));
    if (codes_out) HIPCHK(hipMemcpy(codes_out + offs[0], d_codes.p, nb, hipMemcpyDeviceToHost));
    return 0;
}
