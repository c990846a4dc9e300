// spdp_polya.hip -- PolyA::rmpolyA (ogotoh/spaln v3.0.7 src/seq.cc:1402-1456) for a batch of cDNA queries that lie on the device
// already: the poly-A tail / poly-T head of every query found, its record written, and the queries that turned out to be
// antisense (a T head) reverse-complemented in place, so that the vote and the HSP search read the normalised query.  The
// rule in its sequential form: spdp_polya.h.
//
// One wave per query, blocks of 4 waves.  Both scans are chunked wave scans, 64 residues a step: the A scan runs backwards
// from the 3' end, the T scan forwards from the 5' end.  Per chunk: the inclusive prefix sum of the +1 / -5 terms on top of
// the carried sum, the inclusive running maximum seeded with the carried maximum (0 at the start), a ballot for the first
// lane whose sum has fallen more than thr below the running maximum.  The best score is the running maximum of the last lane
// before the break; its position is the FIRST lane that reaches it (the sequential rule moves only on score > best), and
// lanes at or behind the break never count.  Nearly every query breaks inside its first chunk: both first chunks are
// loaded up front, and nothing loops for them.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "spdp_polya.h"
#include "spdp_wave.h"

namespace {

typedef unsigned long long u64;
constexpr int WAVES = 4;

struct Found { int best; int at; };     // the best score, and the step at which it was first reached (-1: none above thr)

// the scan in one direction; first: the chunk the caller has loaded already (codes of steps 0 .. 63, one per lane).
// code_at(step) reads the residue of a step < n
template <class F>
__device__ __forceinline__ Found scan(F code_at, int first, int n, int base, int thr, int lane)
{
    int sum = 0, top = 0, at = -1;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int step = c0 + lane;
        const bool valid = step < n;
        const int code = c0 == 0 ? first : (valid ? code_at(step) : 0);
        const int s = sum + wave_scan_add(valid ? (code == base ? spdp_polya::MATCH : spdp_polya::MISMATCH) : 0, lane);
        const int m = max(top, wave_scan_max(valid ? s : INT32_MIN, lane));
        const u64 live = __ballot(valid);
        const u64 broke = __ballot(valid && s < m - thr);
        // lanes in front of the break (the breaking lane's own score cannot be a new best: thr > 0)
        const u64 counted = broke ? (live & ((1ull << (__ffsll((long long) broke) - 1)) - 1ull)) : live;
        if (counted) {
            const int last = 63 - __clzll((long long) counted);
            const int chunk_top = __shfl(m, last);
            if (chunk_top > top) {
                const u64 reached = __ballot(s == chunk_top) & counted;
                top = chunk_top; at = c0 + __ffsll((long long) reached) - 1;
            }
            sum = __shfl(s, last);
        }
        if (broke) break;
    }
    return {top, top > thr ? at : -1};
}

__global__ void __launch_bounds__(64 * WAVES) spdp_polya_scan_k(PolyaArgs A)
{
    const int lane = threadIdx.x & 63;
    const int q = __builtin_amdgcn_readfirstlane(blockIdx.x * WAVES + (threadIdx.x >> 6));
    if (q >= A.n) return;
    const int64_t off = A.offs[q];
    const int len = (int) (A.offs[q + 1] - off);
    uint8_t* a = A.codes + off;
    SpdpQueryTail t;
    t.pol = 0; t.tlen = len; t.left = 0; t.right = len; t.ori = A.q_mns;
    t.reserved[0] = t.reserved[1] = t.reserved[2] = 0;
    if (A.thr > 0 && len > 0) {
        const bool t_too = A.q_mns != 1;
        const int tail0 = lane < len ? a[len - 1 - lane] : 0;
        const int head0 = t_too && lane < len ? a[lane] : 0;
        Found fa = scan([&](int i) { return (int) a[len - 1 - i]; }, tail0, len, spdp_polya::CODE_A, A.thr, lane);
        Found ft = {0, -1};
        if (t_too) ft = scan([&](int i) { return (int) a[i]; }, head0, len, spdp_polya::CODE_T, A.thr, lane);
        if (fa.at >= 0 && ft.at >= 0) { if (fa.best >= ft.best) ft.at = -1; else fa.at = -1; }
        if (fa.at >= 0) { t.pol = 1; t.tlen = t.right = len - 1 - fa.at; }
        else if (ft.at >= 0) { t.pol = 2; t.tlen = t.right = len - ft.at; }
    }
    if (t.pol == 2) {
        // Seq::comrev in place: a lane owns the pair (i, len - 1 - i), the middle residue of an odd length its own lane
        for (int i = lane; 2 * i < len; i += 64) {
            const int j = len - 1 - i;
            const uint8_t x = a[i], y = a[j];
            a[i] = spdp_polya::other_strand(y);
            a[j] = spdp_polya::other_strand(x);
        }
    }
    if (lane == 0) A.tails[q] = t;
}

}   // namespace

extern "C" hipError_t spdp_polya_launch(const PolyaArgs* a, hipStream_t s)
{
    if (a->n <= 0) return hipSuccess;
    hipLaunchKernelGGL(spdp_polya_scan_k, dim3((a->n + WAVES - 1) / WAVES), dim3(64 * WAVES), 0, s, *a);
    return hipGetLastError();
}
