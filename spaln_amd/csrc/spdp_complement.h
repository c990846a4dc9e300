// spdp_complement.h -- the other strand of a nucleotide code, for host and device code alike.
// The reference's codes are 1 + the set of bases a letter stands for (A = 1, C = 2, G = 4, T = 8; src/cmn.h), so the complement
// swaps A <-> T and C <-> G inside every set: M <-> K, R <-> Y, H <-> D, V <-> B, while S, W, N and the two pads stay
// (complcod, src/seq.cc:74, which Seq::comrev applies).
#ifndef SPDP_COMPLEMENT_H_
#define SPDP_COMPLEMENT_H_
#include <stdint.h>

#ifdef __HIPCC__
#define SPDP_HOST_DEVICE __host__ __device__
#else
#define SPDP_HOST_DEVICE
#endif

// c = 0 .. 16; a caller that may hold larger codes reads them as 16 first
SPDP_HOST_DEVICE inline int spdp_complement(int c)
{
    constexpr uint8_t other[17] = {0, 1, 9, 5, 13, 3, 11, 7, 15, 2, 10, 6, 14, 4, 12, 8, 16};
    return other[c];
}

#endif
