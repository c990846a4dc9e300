// spdp_polya.h -- what spaln does to every cDNA query before the block search (PolyA::rmpolyA, ogotoh/spaln v3.0.7
// src/seq.cc:1402-1456, called from spaln_job, src/spaln.cc:1154-1166): a poly-A tail is looked for from the 3' end, a poly-T
// head from the 5' end (+1 for the base, -5 for anything else; the best position whose running score is above the threshold,
// the scan given up once the score has fallen more than the threshold below its best); the better of the two stays, A on
// ties.  An A tail clips `right` and sets `tlen`; a T head clips `left` and the query is reverse-complemented in place, so it
// goes on as its own sense strand with an A tail (Seq::rev_attr mirrors the range).
// This header holds the rule in its sequential form (host; no device code: the checker of spdp_polya.hip, the entry
// spdp_polya_scan_host) and the launch of the device form.
#ifndef SPDP_POLYA_H_
#define SPDP_POLYA_H_
#include <stdint.h>
#include "../../include/spdp.h"
#include "spdp_complement.h"

namespace spdp_polya {

enum { CODE_A = 2, CODE_T = 9, MATCH = 1, MISMATCH = -5 };

// one direction: residues read from `first` in steps of `step`, n of them.  -> the step (0-based) at which the best score
// was first reached, or -1 when no score above thr was seen before the scan gave up; *best: that score
inline int64_t scan(const uint8_t* first, int64_t step, int64_t n, int base, int thr, int* best)
{
    int score = 0, top = 0;
    int64_t at = -1;
    for (int64_t i = 0; i < n; ++i) {
        score += first[i * step] == base ? MATCH : MISMATCH;
        if (score > top) { top = score; if (score > thr) at = i; }
        if (score < top - thr) break;
    }
    *best = top;
    return at;
}

// the record of one query of len residues, as it stands after normalisation; -> true when the query has to be reverse-complemented
inline bool decide(const uint8_t* q, int32_t len, int q_mns, int thr, SpdpQueryTail* t)
{
    t->pol = 0; t->tlen = len; t->left = 0; t->right = len; t->ori = q_mns;
    t->reserved[0] = t->reserved[1] = t->reserved[2] = 0;
    if (thr <= 0 || len <= 0) return false;
    int score_a = 0, score_t = 0;
    int64_t a = scan(q + len - 1, -1, len, CODE_A, thr, &score_a);
    int64_t h = q_mns != 1 ? scan(q, 1, len, CODE_T, thr, &score_t) : -1;
    if (a >= 0 && h >= 0) { if (score_a >= score_t) h = -1; else a = -1; }
    if (a >= 0) { t->pol = 1; t->tlen = t->right = (int32_t) (len - 1 - a); }
    else if (h >= 0) { t->pol = 2; t->tlen = t->right = (int32_t) (len - h); }       // (left = h, mirrored by the turn)
    return t->pol == 2;
}

SPDP_HOST_DEVICE inline uint8_t other_strand(uint8_t c) { return c > 16 ? c : (uint8_t) spdp_complement(c); }

}   // namespace spdp_polya

// ---- the device form (spdp_polya.hip): one wave per query, blocks of 4 waves
struct PolyaArgs {
    uint8_t* codes; const int64_t* offs; int32_t n;
    int32_t q_mns, thr;
    SpdpQueryTail* tails;
};
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
extern "C" hipError_t spdp_polya_launch(const PolyaArgs* a, hipStream_t s);
#endif
#endif
