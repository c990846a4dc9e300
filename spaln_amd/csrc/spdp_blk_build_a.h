// spdp_blk_build_a.h -- the per-residue rule of the amino-acid block index (`spaln -W -KA`, <db>.bka), in plain C++ that compiles
// for the device (blkidx_words_a, spdp_blk_build.hip) and for the host (tests/aa_index_host_check.cpp, under the sanitizers).
//
// What the reference keeps as state while it walks a protein database (MakeBlk::scan_genome, src/blksrc.cc:1111-1183, with
// blklen = the longest sequence, so that a block is a sequence; Block::c2w, :448-464; Bitpat_wq::word / flaw, src/bitpat.cc:
// 177-211; WordTab::reset, :439-453), restated for the word that ends at residue g of the packed database:
//     class    = ConvTab[code]: < nalpha a letter's class, nalpha the ambiguous class (residues the scan skips are gone by now)
//     run0     = max(the last ambiguous residue + 1, the sequence's first residue): where the run of g began
//     ss       = g - run0 + 1, a 16-bit counter in the reference (WordTab::ss is a SHORT): it wraps in a run of 65 536
//     flawless = the window of `width` residues lies inside the sequence and every residue the pattern examines has a class
//                (a contiguous pattern: ss >= its weight)
//     word     = sum of class x nalpha^e over the examined residues, the leftmost the most significant
//     phase    = (unsigned) (ss - width) % Nshift == 0          (Nshift is an INT: the reference's remainder is unsigned)
// A flawless word counts in tcount; at its phase it enters the hash of its block, the sequence.
#ifndef SPDP_BLK_BUILD_A_H_
#define SPDP_BLK_BUILD_A_H_
#include <stdint.h>

#ifdef __HIPCC__
#define BLKA_FN __host__ __device__ __forceinline__
#else
#define BLKA_FN inline
#endif

#define BLKA_MAX_K 7

struct BlkRuleA {
    int nalpha, weight, width, spaced, nshift;
    int exam[BLKA_MAX_K];               // the offsets the pattern examines inside its window, leftmost first
    uint8_t cls[32];                    // residue code -> class; >= nalpha: ambiguous
};

struct BlkWordA { bool flawless, emit; uint32_t word; };

// cls: the 32 entries of BlkRuleA::cls, wherever the caller keeps them (the kernel: in LDS)
BLKA_FN int blka_class(const uint8_t* cls, int nalpha, int code)
{
    const int c = cls[code & 31];
    return c < nalpha ? c : nalpha;
}

// x: the classes; x[0] is residue g's own, x[-d] that of the residue d before it (width - 1 of them are readable, whatever they
// hold).  seq_lo: the first residue of g's sequence; last_amb: the last ambiguous residue at or before g (-1: none)
BLKA_FN BlkWordA blka_word(const BlkRuleA& R, const uint8_t* x, int64_t g, int64_t seq_lo, int64_t last_amb)
{
    const int64_t run0 = last_amb + 1 > seq_lo ? last_amb + 1 : seq_lo;
    const int64_t ss = g - run0 + 1;
    BlkWordA o;
    bool ok = g - R.width + 1 >= seq_lo;
    uint32_t w = 0;
    if (R.spaced) {
        for (int e = 0; e < R.weight; ++e) {
            const int c = x[R.exam[e] - (R.width - 1)];
            ok = ok && c < R.nalpha;
            w = w * (uint32_t) R.nalpha + (uint32_t) (c < R.nalpha ? c : 0);
        }
    } else {
        ok = ok && ss >= R.weight;
        for (int e = 0; e < R.weight; ++e) {
            const int c = x[e - (R.weight - 1)];
            w = w * (uint32_t) R.nalpha + (uint32_t) (c < R.nalpha ? c : 0);
        }
    }
    const int nw = (int) (ss & 0xffff) - R.width;
    o.flawless = ok;
    o.emit = ok && (uint32_t) nw % (uint32_t) R.nshift == 0;
    o.word = w;
    return o;
}
#endif
