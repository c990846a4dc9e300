// spdp_blk_finds.hip -- the vote of SrchBlk::finds on the device: ONE QUERY PER WAVE.  The wave's logic is spdp_blk_finds.h
// (shared with the host emulation the tests run under the sanitizers); here are the kernel around it -- the wave's LDS and its area
// of HBM (the slab form or the table form: spdp_blk_finds_dev.h), the queue of queries, the list of queries whose table ran full --
// and the launch.  No MFMA: integer look-ups and compares; the bound is memory latency per word.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "spdp_wave.h"
#define SPDP_FINDS_DEVICE 1
#include "spdp_blk_finds.h"
#include "spdp_blk_finds_dev.h"

namespace {

// HASH: what holds the scores (FindsWave::store) -- 0 the slab of nseg + 1 slots, 1 the table of A.tb_n slots.  A compile-time
// choice, so that the slab form is the code it was
template <int HASH>
__global__ void __launch_bounds__(64) spdp_blk_finds_wave(BlkFindsArgs A)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const BlkDev& X = *A.ix;
    const int me = lane_id();
    FindsWave W;
    W.X = &X; W.lenadj = A.lenadj; W.n_words = A.n_words; W.max_out = A.max_out; W.ptpl = A.ptpl; W.maxmmc = A.maxmmc;
    // ---- LDS: the heap and (when it fits) the run hash first, both of 8-byte entries
    uint32_t* l = lds;
    W.heap = (uint64_t*) l; l += 2 * ((size_t) X.ncand + 1);
    uint64_t* hh_lds = (uint64_t*) l; if (A.hh_in_lds) l += 2 * (size_t) A.hh_n;
    W.st = (int*) l; l += FST_WORDS;
    W.as = (int*) l; l += 2 * 32;
    W.own = l; l += SPDP_FINDS_OWN;
    for (int i = me; i < SPDP_FINDS_OWN; i += 64) W.own[i] = 0xffffffffu;
    // ---- the wave's area: header {tag, epoch}, the scores (rscr: nseg + 1 slots; tb: tb_n slots of two words), stage, the run
    // hash when LDS has no room for it
    uint8_t* g = A.slabs + (size_t) blockIdx.x * A.slab_bytes;
    uint32_t* header = (uint32_t*) g; g += 16;
    const size_t score_words = HASH ? 2 * (size_t) A.tb_n : (size_t) X.nseg + 1;
    uint64_t* scores = (uint64_t*) g; g += 8 * score_words;
    W.store = HASH; W.rscr = HASH ? nullptr : scores; W.tb = HASH ? scores : nullptr;
    W.tb_n = HASH ? A.tb_n : 0u; W.tb_shift = HASH ? 32u - (uint32_t) __builtin_ctz(A.tb_n) : 0u;
    W.stage = (uint32_t*) g; g += 4 * (2 * (size_t) X.maxlist + 2);
    g = (uint8_t*) (((uintptr_t) g + 7) & ~(uintptr_t) 7);
    W.hh = A.hh_in_lds ? hh_lds : (uint64_t*) g;
    W.hh_n = (uint32_t) A.hh_n; W.hh_step = (uint32_t) A.hh_step;
    uint32_t tag = header[0];
    W.epoch = A.hh_in_lds ? 0u : header[1];
    if (A.hh_in_lds) for (uint32_t i = (uint32_t) me; i < W.hh_n; i += 64) W.hh[i] = 0;
    int most = 0;                                       // the most blocks one query of this wave scored
    wave_sync();
    for (;;) {
        int k = 0;
        if (me == 0) k = (int) atomicAdd(A.next, 1u);
        k = __builtin_amdgcn_readfirstlane(k);
        if (k >= A.n) break;
        const int qi = A.which ? A.which[k] : k;        // (a launch that runs listed queries again)
        if (++tag == 0) {                               // (the tags have come round: every slot reads as new again)
            for (size_t i = me; i < score_words; i += 64) scores[i] = 0;
            tag = 1;
            wave_sync();
        }
        W.tag = tag;
        const int64_t o = A.offs[qi];
        const int len = (int) (A.offs[qi + 1] - o);
        const int full = finds_query(W, A.codes + o, len, A.left[qi], A.right[qi], A.out + (size_t) qi * A.out_cap, A.out_cap);
        if (HASH) {
            if (W.n_scored > most) most = W.n_scored;
            if (full && me == 0) A.over[atomicAdd(A.next + 1, 1u)] = qi;       // (at most once per query of the launch: over holds A.n)
        }
        wave_sync();
    }
    if (me == 0) {
        header[0] = tag; header[1] = W.epoch;
        if (HASH) { if ((uint32_t) most > header[2]) header[2] = (uint32_t) most; atomicMax(A.next + 2, (uint32_t) most); }
    }
}

}   // namespace

extern "C" uint32_t spdp_blk_finds_lds_bytes(const BlkDev* ix, int hh_n, int hh_in_lds)
{
    size_t w = 2 * ((size_t) ix->ncand + 1) + FST_WORDS + 2 * 32 + SPDP_FINDS_OWN;
    if (hh_in_lds) w += 2 * (size_t) hh_n;
    return (uint32_t) (4 * w);
}
// tb_n = 0: the slab form
extern "C" size_t spdp_blk_finds_area_bytes(const BlkDev* ix, int hh_n, int hh_in_lds, uint32_t tb_n)
{
    size_t b = 16 + (tb_n ? 16 * (size_t) tb_n : 8 * ((size_t) ix->nseg + 1)) + 4 * (2 * (size_t) ix->maxlist + 2) + 8;
    if (!hh_in_lds) b += 8 * (size_t) hh_n;
    return (b + 255) & ~(size_t) 255;
}
extern "C" hipError_t spdp_blk_finds_launch(const BlkFindsArgs* a, hipStream_t s)
{
    BlkFindsArgs A = *a;
    if (A.tb_n && ((A.tb_n & (A.tb_n - 1)) || !A.over)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(A.next, 0, 16, s);    // the query counter, the overflow counter, the most blocks a query scored
    if (e != hipSuccess) return e;
    if (A.tb_n) hipLaunchKernelGGL(spdp_blk_finds_wave<1>, dim3(A.n_waves), dim3(64), A.lds_bytes, s, A);
    else hipLaunchKernelGGL(spdp_blk_finds_wave<0>, dim3(A.n_waves), dim3(64), A.lds_bytes, s, A);
    return hipGetLastError();
}
