// spdp_b_dev.h -- device-side layout of the unspliced aligner (spdp_b_forward.hip) shared with its host API (spdp_b_api.cpp).
//
// One problem = one wave.  Lane k owns DP row m0 + k of a 64-row tile and the wave sweeps the tile's anti-diagonals: at
// step t lane k computes column nlo + t - k.  Tiles of a problem run one after the other; the last row of a tile passes
// to the next through the problem's row planes (H, F, F2 by column).  HBM arrays, per problem:
//   codes   uint8   residues of a then b, whole sequences (position 0 first)
//   rowp    int32   3 planes of (cols + 1) entries, entry n - b_left: first the top boundary row, then every tile's
//                   last row in place, at the end the DP's last row
//   lastc   int32   rows + 1 entries, entry m - a_left: H of the last column (entry 0: the top boundary's cell)
//   trace   uint8   forward only: one code per cell, tile after tile with a fixed stride of tstride steps; within a tile
//                   the codes of four consecutive steps of a lane share a dword: byte ((t >> 2) * 64 + lane) * 4 + (t & 3)
//   recs    int2    forward only: the path records in Vmf::traceback's order (end -> start), rec_cap per problem
//
// The thin form (spdp_b_sweep_thin, requests of 1 .. 16 rows: what the seeded walk mostly asks for): four requests per wave, one
// per 16-lane DPP row; lane k of a row owns DP row a_left + 1 + k, the request is a single tile, the row above lane 0 is the
// closed-form top boundary.  Per request:
//   rowp    int32   ONE plane of (cols + 1) entries: H of the DP's last row (what lastB_ng reads)
//   lastc   int32   as above
//   trace   uint8   16 x steps4 bytes: the codes of four consecutive steps of a lane share a dword, byte
//                   ((t >> 2) * 16 + k) * 4 + (t & 3) -- a row of lanes stores 64 contiguous bytes every fourth step
#ifndef SPDP_B_DEV_H_
#define SPDP_B_DEV_H_

#include <stdint.h>

#define SPDP_B_TILE 64
// trace code of a cell: bits 0-2 the state H came from, one "opened here" bit per gap state, bit 7: reset to 0 (LocalL)
#define SPDP_B_WIN   7
#define SPDP_B_F_OPEN  0x08
#define SPDP_B_F2_OPEN 0x10
#define SPDP_B_E1_OPEN 0x20
#define SPDP_B_E2_OPEN 0x40
#define SPDP_B_RESET   0x80
enum { SPDP_B_FROM_DIAG = 0, SPDP_B_FROM_F = 1, SPDP_B_FROM_F2 = 2, SPDP_B_FROM_E1 = 3, SPDP_B_FROM_E2 = 4 };

struct DevScoringB {
    int32_t mtx_dim, noll;
    int32_t gop, gep, lgop, lgep;
    int32_t k1;                    // gaps longer than this price with lgop / lgep (LARGEN unless noll == 3)
    int32_t local;
    int32_t mtx[32 * 32];          // stride 32, row / column 0 zero
};

// sum of the boundary penalties of i >= 1 gap positions: first + ext * (those up to k1) + lng * (those beyond)
struct DevEdgeB { int32_t first, ext, lng; };

struct DevProblemB {
    int64_t a_off, b_off;          // into codes
    int64_t row_off;               // into rowp (ints); plane stride = cols + 1
    int64_t col_off;               // into lastc (ints)
    int64_t trace_off;             // into trace (bytes)
    int64_t rec_off;               // into recs (records)
    int32_t a_left, a_right, b_left, b_right;
    int32_t a_len, b_len;
    int32_t lw, up;
    int32_t flags;                 // bit0 a_exgl, bit1 a_exgr, bit2 b_exgl, bit3 b_exgr
    int32_t tstride;               // steps per tile in the trace (multiple of 4)
    int32_t rec_cap;
    DevEdgeB top, left;            // boundary row / column (initB_ng with tgapf folded in; sinitB_ng in score mode)
    DevEdgeB endb, enda;           // lastB_ng: (int)(GapPenalty(1) * f), (int)(BasicGEP * f), (int)(LongGEP * f) for b's / a's right end
    int32_t end_mode;              // bit0: the last-column pass runs, bit1: the last-row pass runs (forward); score mode: b_exgr, a_exgr
    int32_t thin;                  // 1: a request of at most 16 rows in the thin layout (spdp_b_sweep_thin); 0: the tiled layout
};

struct DevResultB {
    int32_t score;
    int32_t best_m, best_n;        // LocalR: the cell of the running maximum
    int32_t n_rec;                 // forward: records written (may exceed rec_cap: then the list is unusable)
};

#endif
