// spdp_internal.h -- declarations shared by spdp_kernels.hip, spdp_api.cpp and spdp_host.cpp
#ifndef SPDP_INTERNAL_H_
#define SPDP_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>
#include "../../include/spdp.h"
#include "spdp_dev.h"
#include "spdp_hostcpus.h"

struct SweepArgs {
    const DevScoring* sc;
    const DevProblem* probs;
    int               n_probs;
    const uint8_t*    a_codes;
    const int2*       cols;
    int*              bnd;        // int2 (score / forward) or int4 (udh) entries
    uint8_t*          tb;         // forward: traceback codes
    int*              imd;        // udh: hlnk0, hlnk1, vlnk0, vlnk1 per intermediate
    DevResult*        res;
    int               n_multi;    // the first n_multi problems get a whole 4-wave block each
    // cross-CU pass pipelines (CROSS kernels): every problem is spread over cross_g blocks
    int               cross_g;    // blocks per problem (0: off)
    int*              gprog;      // per problem: cross_g * WPB progress words, then 2 barrier words; zeroed per launch
    // "every block of this launch has started" (the chunk pipeline of spdp_host.cpp hands the GPU to the next chunk's sweep
    // on it): blocks count themselves in `started` (device, zeroed per launch), the last to arrive sets *started_host (mapped
    // pinned host memory).  Nothing on the device reads either word; both null: no signal (every launch but a gated UDH one)
    unsigned*         started;
    int*              started_host;
};

#if defined(__HIPCC__)
// at the entry of a sweep kernel, ahead of any return: one relaxed add per block, and one plain store by the last arrival
__device__ __forceinline__ void spdp_signal_started(const SweepArgs& A)
{
    if (A.started != nullptr && threadIdx.x == 0) {
        const unsigned before = __hip_atomic_fetch_add(A.started, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (before + 1 == gridDim.x) __hip_atomic_store(A.started_host, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
#endif

#define HIPCHK(call)                                                                     \
    do {                                                                                 \
        hipError_t e_ = (call);                                                          \
        if (e_ != hipSuccess) {                                                          \
            ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                \
            return -1;                                                                   \
        }                                                                                \
    } while (0)

struct WalkArgs {
    const DevProblem* probs;
    int               n_probs;
    const uint8_t*    tb;
    const DevResult*  res;
    int2*             skl;        // per problem: skl_cap records
    int*              n_skl;      // per problem: number of records, -1 on overflow, -2 on bad code
    int               skl_cap;
    int               seq;        // 1: one diagonal step per load (SPDP_WALK_SEQ=1, for A/B runs)
};

#define SPDP_RLST_INHERITED 0x7ffffff0   // pipelined linear-space engines: "rlst as the intermediate rows above left it" (an HLNK value)
struct CposArgs {
    const DevProblem* probs;
    int               n_probs;
    const int*        imd;
    const DevResult*  res;
    int*              cpos;       // per problem cpos_stride ints ((n_im_max + 1) Dim10 rows)
    int*              ranges;     // per problem 4 ints
    int*              scores;
    int               cpos_stride;
    int               strict;     // 1: the -A1 form of the walk (hirschbergS1: r > up, lw <= vlnk)
    int               local;      // 1: local ends (DevResult::ml is the left-end row of the path)
    int*              edge;       // per problem: 1 = the path crosses an intermediate row on or left of the first column, or is
                                  // empty: the one class where the reference's own linear-space result depends on what a previous
                                  // stripe left in its link lanes -- reported, not imitated; may be null
    const int*        pipe;       // pipelined spdp_exact<2>: the sync words of the launch (rlf[] resolves SPDP_RLST_INHERITED), or null
    int               pipe_stride, rlf_off;
};

extern "C" hipError_t spdp_launch_sweep(int flavour, int local, int nquant, int pen_cap, const SweepArgs* args,
                                        int grid, int wpb, hipStream_t s);
// spdp_sweep_fp.hip: the fp32-issue form of the score-only / linear-space sweeps; hipErrorNotSupported = use spdp_launch_sweep
extern "C" int spdp_sweep_fp_serves(int local, int spj, int nquant, int pen_cap, int llmt);
extern "C" hipError_t spdp_launch_sweep_fp(int flavour, int local, int spj, int nquant, int pen_cap, int llmt,
                                           const SweepArgs* args, int grid, int wpb, hipStream_t s);
extern "C" hipError_t spdp_launch_walk(const WalkArgs* a, hipStream_t s);
extern "C" hipError_t spdp_launch_cpos(const CposArgs* a, hipStream_t s);
// exact-intron-length (-A0) engines (spdp_rowwave.hip: one wave per problem, lane = row) and the -A1 engines
#include "spdp_ipen_runs.h"

#define SPDP_VMF_LANE_CHUNK 32      // Vmf record numbers a lane of forwardS1 (spdp_exact<1>) reserves at a time
#ifndef SPDP_VMF_CHUNK
#define SPDP_VMF_CHUNK 512          // Vmf record numbers a wave of a pipelined forwardS_ng problem reserves at a time
#endif
struct ScalarArgs {
    const DevScoring* sc;
    const DevProblem* probs;      // bnd_off = work offset (ints), tb_off = Vmf offset (records), imd_off = Vmf capacity
    int               n_probs;
    const uint8_t*    a_codes;
    const int2*       cols;
    const uint8_t*    aux;        // per position: {bit0 isDonor | bit1 isAccpt, dinc5 << 4 | dinc3}
    const int*        cip;        // Cip_score::cip_score(m) rows of the queries that have one (DevProblem::cip_off), or null
    const int16_t*    intpen;
    int               intpen_len;
    int               ipen;
    const int16_t*    ipen_runs;  // SPDP_IPR_WORDS words (spdp_intpen_runs), or null: long introns read `intpen`
    int               minl;       // IntronPrm.minl (-A1 engines)
    int16_t           t53[256];
    int*              work;
    int3*             vmf;
    DevResult*        res;
    int2*             skl;
    int*              n_skl;
    int               skl_cap;
    // scalar UDH (hirschbergS_ng) only
    int*              imd;        // per problem n_im * 8 * width ints at DevProblem::imd_off
    int*              cpos;       // per problem cpos_stride ints
    int*              ranges;     // per problem 4 ints
    int*              scores;
    int               cpos_stride;
    // tiles of a problem as separate waves (spdp_rowwave<., true>): null = one wave per problem
    int*              pipe;       // per problem pipe_stride ints {records, overflow, prog[max_tiles], best[max_tiles][4]}; then {ticket, stalled}
    int               pipe_stride, pipe_ticket, max_tiles;
    const int2*       items;      // (problem, tile) in dispatch order
    int               n_items;
    // double affine gaps (spdp_rowwave<., ., ., DAGP>): PwdB::Noll, LongGOP, LongGEP, codonk1
    int               noll, lgop, lgep, codonk1;
};
extern "C" hipError_t spdp_launch_rowwave(int forward, const ScalarArgs* a, hipStream_t s);    // spdp_rowwave.hip: -A0 forward / score-only
extern "C" hipError_t spdp_launch_rowwave_udh(const ScalarArgs* a, hipStream_t s);            // spdp_rowwave.hip: -A0 linear space
extern "C" hipError_t spdp_launch_local_udh(const ScalarArgs* a, hipStream_t s);          // spdp_local_udh.hip: hirschbergS1_wip, -LS
extern "C" hipError_t spdp_launch_exact(int mode, const ScalarArgs* a, hipStream_t s);   // spdp_exact.hip: 0 score, 1 forward, 2 udh
extern "C" hipError_t spdp_launch_pack(const int2* skl, int skl_cap, const int* n_skl, const int64_t* off,
                                       int2* packed, int n_probs, hipStream_t s);

// splice-signal precompute (spdp_signals.hip): Exinon::intron53_c / intron53_n per position of a genomic window
struct SigModelDev {
    int32_t rows, cols5, off5, cols3, off3, any, both_ori;
    float   fs, tonic5, min5, tonic3, min3;
    int16_t tab5[16], tab3[16];
};
struct SigJob {
    int64_t b_off;                // first base of the window in `codes`
    int64_t col_off;              // its column records (DevStore layout)
    int64_t out_off;              // its plain output arrays
    int32_t b_len, left, right, pad;
};
struct SignalArgs {
    const SigModelDev* model;
    const float*       mtx5;      // cols5 x rows
    const float*       mtx3;
    const SigJob*      jobs;
    const uint8_t*     codes;
    int16_t*           sig5;      // plain arrays, b_len + 1 entries per job at out_off (or null)
    int16_t*           sig3;
    uint8_t*           cano5;
    uint8_t*           cano3;
    uint8_t*           dinc;
    int2*              cols;      // column records / aux of the sweeps (or null)
    uchar2*            aux;
    int*               maxes;     // {max(sig5 + ipen), max sig3} over everything written (or null)
    int32_t            ipen, spj;
};
int spdp_signals_run(SpdpContext* ctx, const SpdpSignalModel* m, const std::vector<SigJob>& jobs, SignalArgs args,
                     int* max_s5, int* max_s3);          // spdp_signals_api.cpp
extern "C" hipError_t spdp_launch_signals(const SignalArgs* a, int n_jobs, int max_len, int lds_floats, hipStream_t s);

// skl_rngS_ng on the device (spdp_rescore.hip): one thread per query
struct RescoreArgs {
    const DevScoring* sc;
    const DevProblem* probs;
    int               n_probs;
    const uint8_t*    a_codes;
    const int2*       cols;
    const uint8_t*    aux;
    const int16_t*    intpen;
    int               intpen_len;
    const int2*       skl;        // corner lists without header, query i at skl_off[i], skl_cnt[i] corners
    const int64_t*    skl_off;
    const int*        skl_cnt;
    const int64_t*    rec_off;    // first exon record of query i (21 ints each)
    int*              out_hdr;    // per query 8 ints: h, mch, mmc, gap, unp, val, n_records, 0
    int*              out_rec;
    int               gop, gep, lgop, lgep, codonk1, minl, jneibr, lsg, ipen;
    int16_t           t53[256];
    // edit records for the Cigar / Vulgar / SAM writers (0: none)
    int               ops_format; // 1 Cigar, 2 Vulgar, 3 SAM
    int3*             ops;        // query i: records at ops_off[i] .. ops_off[i + 1]
    const int64_t*    ops_off;
    int*              ops_cnt;    // records the walk produced (may exceed the slot: then the slot is full and the rest lost)
    const int*        a_len;      // SAM: query lengths
    const int*        cip;        // Cip_score::cip_score(m) rows (DevProblem::cip_off), or null: the bonus of use_spb()
    const int*        a_len_all;  // query lengths (always set when cip is)
};
extern "C" hipError_t spdp_launch_rescore(const RescoreArgs* a, hipStream_t s);

// skl_rngH_ng on the device
struct HRescoreProb {
    int32_t a_left, a_right, b_left, b_right;
    int32_t a_len, b_len;
    int32_t a_exgl, a_exgr, b_exgl, b_exgr;
    int64_t a_off, b_off, col_off;
    int32_t w_lo, w_hi;               // the region positions the launch holds: [w_lo, w_hi) of the problem's b_len + 3 (the corners' span and a margin)
};
struct HRescoreArgs {
    const int*        mtx;        // stride 32: mtx[aa * 32 + tron]
    int               n_probs;
    const HRescoreProb* probs;
    const uint8_t*    a_codes;
    const uint8_t*    b_codes;    // tron codes, b_len + 1 per problem
    const short*      sig;        // per position 5 shorts: sig5, sig3, sigS, sigT, sigE
    const int8_t*     phs;        // per position 2: phs5, phs3
    const uint8_t*    dinc;
    const int16_t*    intpen;
    int               intpen_len;
    const int2*       skl;
    const int64_t*    skl_off;
    const int*        skl_cnt;
    const int64_t*    rec_off;
    int*              out_hdr;
    int*              out_rec;
    int               gop, gep, lgop, lgep, codonk1, gape1, gape2, extragop, diffu, k1;
    int               minl, jneibr, lcl, sup_tcodon;
    int16_t           t53[256];
    uint8_t           mid[32];    // tron code -> its codon's middle base (0..3), 4 = ambiguous
    uint8_t           tron_of[64];// codon (A C G T order) -> tron code
    // edit records for the Cigar / Vulgar writers (0: none; 1 Cigar, 2 Vulgar), as RescoreArgs
    int               ops_format;
    int3*             ops;
    const int64_t*    ops_off;
    int*              ops_cnt;
};
extern "C" hipError_t spdh_launch_rescore(const void* args, hipStream_t s);

// grow-only device allocations reused across launches (hipMalloc / hipFree of multi-GB
// work buffers per batch costs seconds)
struct DevPool {
    enum { N_SLOTS = 16 };
    void*  ptr[N_SLOTS] = {nullptr};
    size_t cap[N_SLOTS] = {0};
    void*  get(int slot, size_t bytes);
    void   release();
};
enum { POOL_PROBS = 0, POOL_BND, POOL_TB, POOL_IMD, POOL_RES, POOL_SKL, POOL_NSKL, POOL_CPOS,
       POOL_RANGES, POOL_SCORES, POOL_SKLPACK, POOL_SKLOFF, POOL_GPROG };

// an on / off knob of the environment: unset or non-zero = on.  Read on every call (the tests flip knobs between calls)
static inline bool spdp_knob_on(const char* name) { const char* e = getenv(name); return !e || atoi(e) != 0; }

// a blocking copy.  hipMemcpy goes through the null stream, which first waits for every blocking stream of the process.
// With t_lane_copies set the copy waits for its OWN stream only: in the request batches of the seeded path
// (spdp_run_requests / spdh_run_requests) and on the chunk lanes of align_on_store (spdp_host.cpp; SPDP_CHUNK_LANE_COPIES).
// What then orders a lane's copies: a copy goes through DevRun::strm(), the stream of the run's uploads and launches,
// and every fetch follows DevRun::sync(), a host wait for that stream (side runs: side.sync()).  Lanes share no buffer
// (spdp_lane); the one dependency between them is the gate's (ChunkGate: an event or the start signal).  An async copy
// to or from a pageable vector is waited for before the vector is used or freed.  Everywhere else: the null-stream form.
extern thread_local bool t_lane_copies;
struct LaneCopies {
    bool was;
    explicit LaneCopies(bool on = true) : was(t_lane_copies) { t_lane_copies = was || on; }
    ~LaneCopies() { t_lane_copies = was; }
};
static inline hipError_t spdp_copy_sync(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t s)
{
    if (!t_lane_copies) return hipMemcpy(dst, src, n, kind);
    const hipError_t e = hipMemcpyAsync(dst, src, n, kind, s);
    return e != hipSuccess ? e : hipStreamSynchronize(s);
}

// Host side of the tile / stripe pipelines of the -A0 and -A1 engines, cDNA and protein alike (device side: spdp_pipe.h,
// on the wave helpers of spdp_wave.h).
// The tiles of a problem run as a pipeline of waves: the work list (problem, tile) in dispatch order lies behind the sync
// words of the problems and their {ticket, stalled} pair.  A wave that waited in vain for the tile above it leaves a mark,
// and the caller repeats the launch without the pipeline.  Whether a pipeline is wanted (SPDP_A0_PIPE, SPDP_A1_PIPE,
// SPDP_HX_PIPE, cut ranges, Noll = 3) is the caller's decision.
//
// Sync words per problem (`stride`, mt = max_tiles): {records, overflow}, prog[mt], best[mt][.], and what the
// intermediate rows of a linear-space run hand down:
//                      -A0 forward / score   -A0 linear space        -A1 (max_im = 0 unless linear space)
//   cDNA  (ScalarArgs)   2 + 5 mt              2 + 9 mt + max_im       2 + 7 mt + max_im
//   aa    (HScalarArgs)  2 + 9 mt              2 + 9 mt + 3 max_im     2 + 7 mt + 3 max_im
// The 2 and the multipliers of mt (words per tile: prog + best[.]), as pipe_words() of spdp_pipe.h carves the words up:
enum { SPDP_PIPE_HDR = 2, SPDP_PIPE_TPW_A0 = 5, SPDP_PIPE_TPW_A0_UDH = 9, SPDP_PIPE_TPW_A1 = 7, SPDP_PIPE_TPW_H_A0 = 9, SPDP_PIPE_TPW_H_A1 = 7 };
struct TilePipe {
    std::vector<int> items;                 // (problem or group, tile) pairs in dispatch order
    int max_tiles = 1;                      // most tiles of one problem
    int stride = 0;                         // sync words per problem
    int rlf_off = 0;                        // of these, where the words of the intermediate rows start
    size_t words = 0;                       // sync words ahead of the item list
    int* d = nullptr;                       // words, then items (owned by the pool reserve() took it from)
    bool on = false;

    void add(int j, int nt) { max_tiles = std::max(max_tiles, nt); for (int t = 0; t < nt; ++t) { items.push_back(j); items.push_back(t); } }
    // -A0: problem j's tiles of th rows; rows = from the first tiled row to a_right
    void plan(int j, int rows, int th) { add(j, std::max(1, (rows + th) / th)); }          // as the kernel counts them
    // -A1: a work item is (G consecutive problems, stripe of 16 rows)
    template <class Prob> void plan_groups(const std::vector<Prob>& probs, int G)
    {
        const int n = (int) probs.size();
        for (int q = 0; q * G < n; ++q) {
            int ns = 1;
            for (int j = q * G; j < std::min(n, (q + 1) * G); ++j) ns = std::max(ns, (probs[j].a_right - probs[j].a_left + 15) / 16);
            add(q, ns);
        }
    }
    // the device words of n problems of an engine with tpw words per tile (SPDP_PIPE_TPW_*) and `extra` words for its
    // intermediate rows; false = out of device memory
    bool reserve(DevPool& pool, int slot, int n, int tpw, int extra)
    {
        rlf_off = SPDP_PIPE_HDR + tpw * max_tiles;
        stride = rlf_off + extra;
        words = ((size_t) n * stride + 2 + 1) & ~(size_t) 1;
        d = (int*) pool.get(slot, sizeof(int) * (words + items.size()));
        return on = d != nullptr;
    }
    // ahead of every launch: clears the words, copies the work list, sets the kernel's six fields (pipe = null when off)
    template <class Args> hipError_t arm(hipStream_t s, int n, Args& A) const
    {
        A.pipe = nullptr;
        if (!on) return hipSuccess;
        hipError_t e = hipMemsetAsync(d, 0, sizeof(int) * words, s);
        if (e == hipSuccess) e = hipMemcpyAsync(d + words, items.data(), sizeof(int) * items.size(), hipMemcpyHostToDevice, s);
        A.pipe = d; A.pipe_stride = stride; A.pipe_ticket = n * stride; A.max_tiles = max_tiles;
        A.items = (const int2*) (d + words); A.n_items = (int) (items.size() / 2);
        return e;
    }
    // after the launch has finished: *gave_up = a wave gave up (repeat without the pipeline), or the test hook asks for the repeat
    hipError_t stalled(hipStream_t s, int n, bool* gave_up) const
    {
        int mark[2] = {0, 0};
        const hipError_t e = on ? spdp_copy_sync(mark, d + (size_t) n * stride, sizeof mark, hipMemcpyDeviceToHost, s) : hipSuccess;
        *gave_up = on && (mark[1] != 0 || getenv("SPDP_A0_PIPE_TEST_STALL"));
        return e;
    }
};

// SpdpContext::pool: runs that may be in flight together never share one.  The first five: DevRun's (RUN_TRAITS below); H_POOL / HU_POOL: the
// aa x genome path's inputs + traceback runs / linear-space runs; R_POOL: rescoring; SIDE_POOL: a DevRun on the side stream, of any flavour;
// B_POOL: the unspliced aligner (spdp_b_api.cpp)
// slots of pool[B_POOL]: a chunk of spdp_align_b / spdp_homscore_b or a round of spdp_align_b_seeded (never both at once on one
// context), and the residues of a seeded call's pairs, resident for the whole call
enum { BP_SC = 0, BP_PROBS, BP_CODES, BP_ROWP, BP_LASTC, BP_TRACE, BP_RECS, BP_RES, BP_RESIDENT };
enum CtxPool { WIP_SCORE_POOL = 0, WIP_FORWARD_POOL, WIP_UDH_POOL, EXACT_FORWARD_POOL, EXACT_POOL, H_POOL, HU_POOL, R_POOL, SIDE_POOL, B_POOL, N_CTX_POOLS };
struct SpdpContext {
    DevPool pool[N_CTX_POOLS];
    int device = 0;
    int n_cu = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipStream_t stream2 = nullptr;   // side stream (non-blocking): a forward run beside the linear-space rounds
    hipEvent_t ev2 = nullptr, ev3 = nullptr;
    std::string name;
    std::string err;
    std::vector<SpdpContext*> lanes;  // further lanes of this context (spdp_lane): chunks of a batch run side by side
    int64_t seed_stats[12] = {0};      // spdp_seeded_stats
    int64_t seed_stats_b[16] = {0};    // spdp_seeded_stats_b
    int64_t finds_stats[8] = {0};      // spdp_blk_finds_stats: the last spdp_map_align_b call (spdp_map_b_api.cpp)
    int64_t finds_store[8] = {0};      // spdp_blk_finds_store_stats: the last spdp_blk_finds[_resident] call (spdp_blk_finds_api.cpp)
    int64_t hsp_stats[8] = {0};        // spdp_blk_find_stats: the HSP searches of the last block search (spdp_blk_api.cpp, HspBatch::run)
    // Seq::tlen of the problems of the seeded calls made while it is set (spdp_map_align_s_prep; problem i of spdp_align_s_seeded,
    // forward problems then reverse ones of _ori3): the walks' own HSP searches end their forward extension there.  Null: a_len
    const int32_t* seed_a_tlen = nullptr;
    std::vector<std::vector<SpdpPhaseMark>> seed_marks;    // spdp_seeded_phase_marks: per query of the last spdp_align_h_seeded call
    int64_t rerun_stats[2] = {0, 0};   // launches repeated because a cross-CU group / a tile pipeline gave up (spdp_rerun_stats)
    // launches of the `_wip` sweeps (the FAM_WIP flavours of DevRun::launch, repeats included): served by spdp_sweep_fp, served by
    // spdp_sweep, with cross-CU groups, as 16-wave blocks (spdp_sweep_stats; atomic: a side-stream run launches from its own thread)
    std::atomic<int64_t> sweep_stats[4] = {};
    // the "all blocks started" words of a gated sweep launch (SweepArgs::started / started_host): one pair per lane, allocated
    // on the first such launch; sig_host is mapped pinned memory the chunk's thread polls, sig_host_dev its device address
    unsigned* d_started = nullptr;
    int*      sig_host = nullptr;
    int*      sig_host_dev = nullptr;
    int       start_signal();           // allocates the words once: 0, or -1 with err set
    // chunk pipeline of the align calls on this context (spdp_chunk_stats): calls, chunks, gates opened by the start
    // signal / by the recorded event / with nothing to wait for, gates opened exactly once
    std::atomic<int64_t> chunk_stats[6] = {};
    void*  stage_ptr[3] = {nullptr, nullptr, nullptr};   // pinned host staging (grow-only): [0], [1] DevStore::upload, [2] the regions and
    size_t stage_cap[3] = {0, 0, 0};                     // signal arrays of spdp_map_align_s
    void*  staging(int k, size_t bytes);
};
SpdpContext* spdp_lane(SpdpContext* ctx, int i);

// Column records of problems 0 .. off.size() - 1 to the device through the context's pinned staging (spdp_api.cpp).  Problem i
// holds positions off[i] .. off[i + 1] (tot after the last) of every stream.  The problems are cut into groups of at least
// grp_positions positions, and the groups go through a ring of four slots of the staging: a group is copied as soon as its problems
// are packed, and its slot is packed again once that copy has left.  pack(i, at) fills problem i's records at position `at` of every
// stream's staging (StagedStream::host); it runs once per problem, on threads the function starts.  Returns once the copies are
// done (the staging is the context's): 0, or -1 with ctx->err set.
struct StagedStream {
    int    slot;                // SpdpContext::staging slot
    void*  dev;                 // position p's record at dev + p * bytes
    size_t bytes;               // per position
    void*  host = nullptr;      // set before the first pack(): the slot's memory
};
int spdp_upload_ring(SpdpContext* ctx, const std::vector<int64_t>& off, int64_t tot, int64_t grp_positions,
                     std::vector<StagedStream>& st, const std::function<void(int i, int64_t at)>& pack);
// conserved-intron bonus rows (SpdpProblem::cip, SpdpProblemH::cip) to one device array *d (hipMalloc, the caller frees it):
// row(i, len) is problem i's row of len ints, or null; off[i] = where it starts in *d, -1 = none.  Returns 0, or -1 with ctx->err set
int spdp_upload_cip(SpdpContext* ctx, int n, const std::function<const int32_t*(int i, size_t& len)>& row, std::vector<int32_t>& off,
                    void** d);

// Resident inputs of a set of parent problems: residues, per-position column
// records and the scoring bundle.  Sub-problems (UDH slabs, engine calls on
// sub-ranges) are descriptors pointing into these arrays -- no re-upload.
struct DevStore {
    SpdpContext* ctx = nullptr;
    SpdpScoring sc;
    int n_parents = 0;
    std::vector<int64_t> a_off, col_off;
    std::vector<int32_t> a_len, b_len;
    void *d_sc = nullptr, *d_a = nullptr, *d_cols = nullptr, *d_aux = nullptr, *d_intpen = nullptr, *d_cip = nullptr;
    void* d_ipen_runs = nullptr;            // spdp_intpen_runs() of the table, when it has that shape
    std::vector<int32_t> cip_off;           // per parent: first entry of its cip row in d_cip, -1 = none
    bool has_exact = false;                 // exact-model inputs (cano / dinc / intpen) were supplied
    int fp_maxpos = 1, fp_gain = 0;         // largest substitution score; best net score of one intron (>= 0)
    int max_s5 = INT32_MIN, max_s3 = INT32_MIN;   // largest sig5 + ipen / sig3 of the column records (what fp_gain was made from)
    DevStore() = default;
    DevStore(const DevStore&) = delete;
    DevStore& operator=(const DevStore&) = delete;
    ~DevStore() { release(); }
    int upload(SpdpContext* c, const SpdpScoring* sc, const SpdpProblem* probs, int n);
    void release();
};

// one DP call on (a sub-range of) a parent problem
struct RunItem {
    int parent;
    int a_left, a_right, b_left, b_right;
    uint8_t a_exgl, a_exgr, b_exgl, b_exgr;
    SpdpWindow w;
    int n_im;          // UDH only
    int imd_intvl = 0; // scalar UDH only: Aln2s1::imd_intvl as lspS_ng set it
    int vmf_scale = 1; // Vmf-backed forward runs: 1 = the usual record budget, larger on the retry after an overflow
    int cut_l = 0, cut_r = 0;   // scalar forward only: forwardS_ng's cut range (cut_r > cut_l), see spdp_rowwave<1, false, true>
};

// The engines a DevRun drives.  SPDP_TRACE_RUNS prints the number; DESIGN.md section 5 has the table with kernels and outputs.
enum RunFlavour : int { RUN_WIP_SCORE = 0, RUN_WIP_FORWARD, RUN_WIP_UDH, RUN_A0_FORWARD, RUN_A0_SCORE, RUN_A0_UDH,
                        RUN_A1_SCORE, RUN_A1_FORWARD, RUN_A1_UDH, RUN_LOCAL_UDH, RUN_N_FLAVOURS };
enum RunFamily : uint8_t { FAM_WIP, FAM_A0, FAM_A1, FAM_LOCAL };
enum RunKind : uint8_t { KIND_SCORE, KIND_FORWARD, KIND_UDH };
enum RunLauncher : uint8_t { BY_SWEEP, BY_ROWWAVE, BY_ROWWAVE_UDH, BY_EXACT, BY_LOCAL_UDH };
struct RunTraits {
    RunFamily   family;
    RunKind     kind;
    CtxPool     pool;       // of a run on the main stream: flavours that share one are never in flight together
    bool        vmf;        // the traceback is kept as Vmf records (tb = int3 records, DevProblem::imd_off = the problem's budget)
    bool        edge;       // spdp_udh_cpos walks the links after the sweep and leaves CposArgs::edge
    uint8_t     bw;         // ints per entry of the boundary / work buffer
    uint8_t     pipe_tpw;   // tile pipeline: sync words per tile (SPDP_PIPE_TPW_*), 0 = the engine has none
    RunLauncher launcher;
    int         arg;        // its flavour / forward / mode argument
    constexpr bool records() const { return kind == KIND_FORWARD; }     // a record list per problem (skl, n_skl)
    constexpr bool rows() const { return kind == KIND_UDH; }            // intermediate rows in, cpos / ranges / scores out
};
inline constexpr RunTraits RUN_TRAITS[RUN_N_FLAVOURS] = {
    //                    family     kind          pool                vmf    edge  bw  pipe_tpw              launcher
    /* RUN_WIP_SCORE   */ {FAM_WIP,   KIND_SCORE,   WIP_SCORE_POOL,     false, false, 2, 0,                    BY_SWEEP,       0},
    /* RUN_WIP_FORWARD */ {FAM_WIP,   KIND_FORWARD, WIP_FORWARD_POOL,   false, false, 2, 0,                    BY_SWEEP,       1},
    /* RUN_WIP_UDH     */ {FAM_WIP,   KIND_UDH,     WIP_UDH_POOL,       false, true,  4, 0,                    BY_SWEEP,       2},
    /* RUN_A0_FORWARD  */ {FAM_A0,    KIND_FORWARD, EXACT_FORWARD_POOL, true,  false, 1, SPDP_PIPE_TPW_A0,     BY_ROWWAVE,     1},   // (2 over cut ranges)
    /* RUN_A0_SCORE    */ {FAM_A0,    KIND_SCORE,   EXACT_POOL,         false, false, 1, SPDP_PIPE_TPW_A0,     BY_ROWWAVE,     0},
    /* RUN_A0_UDH      */ {FAM_A0,    KIND_UDH,     EXACT_POOL,         false, false, 1, SPDP_PIPE_TPW_A0_UDH, BY_ROWWAVE_UDH, 0},
    /* RUN_A1_SCORE    */ {FAM_A1,    KIND_SCORE,   EXACT_POOL,         false, false, 1, SPDP_PIPE_TPW_A1,     BY_EXACT,       0},
    /* RUN_A1_FORWARD  */ {FAM_A1,    KIND_FORWARD, EXACT_FORWARD_POOL, true,  false, 1, SPDP_PIPE_TPW_A1,     BY_EXACT,       1},
    /* RUN_A1_UDH      */ {FAM_A1,    KIND_UDH,     EXACT_POOL,         false, true,  1, SPDP_PIPE_TPW_A1,     BY_EXACT,       2},
    /* RUN_LOCAL_UDH   */ {FAM_LOCAL, KIND_UDH,     EXACT_POOL,         false, true,  1, 0,                    BY_LOCAL_UDH,   0},
};

// Vmf record budget of one forwardS_ng / forwardS1 call over rows x cols cells in a band of `width` (spdp_api.cpp)
int64_t vmf_capacity(int64_t rows, int64_t cols, int64_t width, int64_t scale);

// descriptors + work buffers of one run of one engine (RunFlavour) over a DevStore
struct ItemShare;
struct DevRun {
    SpdpContext* ctx = nullptr;
    SpdpContext* use_ctx = nullptr;         // set before build: the lane to run on (default: the store's context)
    const DevStore* store = nullptr;
    RunFlavour flavour = RUN_WIP_SCORE;
    int n = 0;
    int n_multi = 0;                        // leading problems run as multi-wave pipelines
    int wpb = 4;                            // waves per block of the sweep launch (16: one huge problem per CU)
    int cross_g = 0;                        // > 0: every problem spread over this many 16-wave blocks (CUs)
    bool fp_ok = false;                     // scores stay inside the exact fp32 range: spdp_sweep_fp.hip may run it
    void* d_gprog = nullptr;                // progress / barrier words of the cross-CU pipelines
    bool cut = false;                       // RUN_A0_FORWARD with cut ranges on every item (set by build)
    TilePipe pipe;                          // -A0 tiles / -A1 stripes of a problem as separate waves: shares POOL_GPROG with d_gprog
    int max_n_im = 0, max_skl = 0;
    int64_t total_cells = 0, tb_bytes = 0;
    std::vector<DevProblem> h_probs;        // in dispatch order
    std::vector<int> order;                 // dispatch slot -> caller index
    void *d_probs = nullptr, *d_bnd = nullptr, *d_tb = nullptr, *d_imd = nullptr, *d_res = nullptr,
         *d_skl = nullptr, *d_nskl = nullptr, *d_cpos = nullptr,
         *d_ranges = nullptr, *d_scores = nullptr;         // all owned by pool()
    int skl_cap = 0;
    float kernel_ms = 0.f;
    bool side = false;                      // run on ctx->stream2 (set before build)
    bool in_flight = false;                 // launched, not yet waited for
    bool signal_start = false;              // set before launch: arm the "all blocks started" signal where the launch can carry it
    bool signal_armed = false;              // set by launch_sweep: this launch carries it (ctx->sig_host)
    bool beside = false;                    // another kernel fills the GPU meanwhile: keep to 4-wave blocks (a 16-wave
                                            // block finds no CU with room while small blocks keep refilling them)
    hipStream_t strm() const { return side ? ctx->stream2 : ctx->stream; }
    hipEvent_t evb() const { return side ? ctx->ev2 : ctx->ev0; }
    hipEvent_t eve() const { return side ? ctx->ev3 : ctx->ev1; }
    explicit DevRun(SpdpContext* lane = nullptr) : use_ctx(lane) {}
    DevRun(const DevRun&) = delete;
    DevRun& operator=(const DevRun&) = delete;
    ~DevRun() { release(); }
    const RunTraits& traits() const { return RUN_TRAITS[flavour]; }
    DevPool& pool() const { return ctx->pool[side ? SIDE_POOL : traits().pool]; }
    void* take(int slot, size_t bytes);                         // pool().get, or null with ctx->err set
    int cpos_stride() const { return 10 * (max_n_im + 1); }     // ints of a problem's cpos output: max_n_im + 1 Dim10 rows
    int build(const DevStore* st, const std::vector<RunItem>& items, RunFlavour flav);
    // the steps of build(), in its order
    int check();
    int lay_out(const std::vector<RunItem>& items, ItemShare& tot);
    int allocate(const ItemShare& tot);
    void sort_dispatch(bool may_multi);
    int plan_blocks(bool may_multi);    // n_multi, wpb, cross_g and the gprog words
    int plan_pipe();
    int launch();                       // async on ctx->stream: launch_sweep (+ walk) or launch_scalar, then the link walk (cpos_args)
    int launch_sweep(), launch_scalar();
    CposArgs cpos_args(int strict, int local, const int* pipe_words) const;
    int sync();                         // waits, fills kernel_ms
    int fetch_results(std::vector<DevResult>& out);
    // forward: records of problem i are skl[off[i] .. off[i] + n_skl[i])
    int fetch_skl(std::vector<int>& n_skl, std::vector<int64_t>& off, std::vector<SpdpSkl>& skl);
    int fetch_udh(std::vector<int32_t>& scores, std::vector<int32_t>& cpos, std::vector<int32_t>& ranges,
                  std::vector<int32_t>* edge = nullptr);     // edge: CposArgs::edge per problem (RunTraits::edge), zeros otherwise
    void release();
};

RunItem spdp_item_of(const SpdpProblem& p, int parent, int sh);
// explicit engine calls on sub-ranges of store entries (spdp_host.cpp: spdp_run_requests); all arrays indexed by request
struct SpdpRequests {
    const int* parents;            // store entry
    const SpdpWindow* windows;
    const uint8_t* kinds;          // 0 lspS_ng, 1 trcbkalignS_ng, 2 trcbkalignS_ng with a cut range
    const int* cuts;               // 2 per request: cut_l, cut_r (kind 2)
};
int spdp_run_requests(SpdpContext* ctx, const DevStore* st, const SpdpProblem* probs, int n, const SpdpRequests* req,
                      SpdpAlignment* out);
void trim_skl_of(std::vector<SpdpSkl>& s, const SpdpProblem& p);     // trimskl, src/gaps.cc:254-273
int64_t spdp_cells_w(int a_left, int a_right, int b_left, int b_right, const SpdpWindow& w);
// corner list of path records (spdp_host.cpp): M_UNIT = 1 nucleotide rows, 3 protein rows
template <int M_UNIT> std::vector<SpdpSkl> corner_list(std::vector<SpdpSkl> pts);

// ---- the unspliced aligner's requests on resident inputs (spdp_b_api.cpp; the seeded entry spdp_seeded_b.cpp asks) ----------
// The residues of a call's pairs go to the device once (spdp_b_resident_open); a round of lspB_ng requests -- sub-ranges of those
// pairs with their own end flags -- is then served in one go: the branches without a DP cell on the host, requests of at most
// 16 rows by the thin sweep (unless SPDP_B_THIN=0), the others by the tiled sweep, in sub-rounds whose trace stores fit
// max_trace_bytes.  A request above the budget comes back with status 1 ("not computed").  The thin requests of a launch set run
// sorted by step count, four of a kind per wave, unless SPDP_B_THIN_SORT=0 (then in the order given).
struct SpdpBRequest {
    int parent = 0;                 // the pair
    SpdpProblem p{};                // the pair's sequences (host pointers) with the request's ranges and end flags
    SpdpWindow w{};
    int score = SPDP_NEVSEL;
    int status = 0;                 // 0: served, 1: above max_trace_bytes
    std::vector<SpdpSkl> rec;       // what lspB_ng wrote, in its order
};
struct SpdpBResident { std::vector<int64_t> a_off, b_off; };
// [0] device launches (sub-rounds), [1] thin requests, [2] tiled requests, [3] served without a cell, [4] requests of at most 16
// rows, [5] their cells, [6] cells of all device requests, [7] requests not computed
enum { SPDP_BREQ_N_STATS = 8 };
int spdp_b_resident_open(SpdpContext* ctx, const SpdpScoring* sc, const SpdpProblem* probs, int n, SpdpBResident* res);
int spdp_b_run_requests(SpdpContext* ctx, const SpdpScoring* sc, const SpdpUnsplicedParams* up, const SpdpBResident* res,
                        SpdpBRequest* const* reqs, int n, int64_t* stats);
const char* spdp_b_refused(const SpdpScoring* sc, const SpdpUnsplicedParams* up);
const char* spdp_b_bad_problem(const SpdpScoring* sc, const SpdpProblem* p);

#endif
