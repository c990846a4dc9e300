// spdp_pipe.h -- device side of TilePipe (spdp_internal.h): what the five kernels whose tiles / stripes run as a pipeline of
// waves (spdp_rowwave, spdp_rowwave_udh, spdh_rowwave, spdp_exact, spdh_exact) share of that protocol.  A wave draws a work
// item from the ticket counter, so a tile's predecessor is always resident or done; the arrays the tiles share cross CUs
// (gld / gst<true>, spdp_wave.h); a tile publishes how far it has handed its entries back once its stores have drained, and
// waits for the word of the tile above before it reads.
// Here: where a problem's sync words lie, and the publish.  The ticket draw, the wait and the Vmf record allocators are
// still written out in each kernel, on the helpers of spdp_wave.h: as functions they compute the same, but the compiler
// lays the sweep around them out differently (MEASUREMENTS.md has the sizes), and these kernels are at their register
// budgets -- they move here once that layout has been timed.  Keep the copies in step until then.
#ifndef SPDP_PIPE_H
#define SPDP_PIPE_H
#include "spdp_internal.h"
#include "spdp_wave.h"

// the sync words of problem pi as TilePipe laid them out; TPW: the engine's SPDP_PIPE_TPW_* (spdp_internal.h)
template <bool PIPE, int TPW, class Args>
__device__ __forceinline__ void pipe_words(const Args& A, int pi, int*& sy, int*& prog, int*& tbest, int*& rlf)
{
    sy = PIPE ? A.pipe + (size_t) pi * A.pipe_stride : nullptr;
    prog = PIPE ? sy + SPDP_PIPE_HDR : nullptr;
    tbest = PIPE ? sy + SPDP_PIPE_HDR + A.max_tiles : nullptr;
    rlf = PIPE ? sy + SPDP_PIPE_HDR + TPW * A.max_tiles : nullptr;
}

// what this wave stored is out before the word says so; one lane (of the wave, or of each group) stores the word
__device__ __forceinline__ void pipe_publish(int* word, int v, bool i_store)
{
    stores_drained();
    if (i_store) gst<true>(word, v);
}

#endif
