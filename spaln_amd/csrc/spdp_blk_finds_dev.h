// spdp_blk_finds_dev.h -- what the finds vote's kernel (spdp_blk_finds.hip) and its host side (spdp_blk_finds_api.cpp) share, and
// what the host side asks of the resident index (spdp_blk_api.cpp).  Data only.
#ifndef SPDP_BLK_FINDS_DEV_H_
#define SPDP_BLK_FINDS_DEV_H_
#include "spdp_blk_dev.h"

// WHAT HOLDS rscr.  The reference keeps rscr[nseg] per thread and clears it per query.  Here a wave owns an area of HBM, in one of
// two forms, and in both a score is a {query tag, value} word that an earlier query's tag makes read as 0, so nothing is cleared
// between queries (the tags come round after 2^32 - 1 queries of a wave; the wave then wipes its scores once):
//   * THE SLAB: nseg + 1 slots, a block's slot at its number -- one load and one store per posting entry, 8 bytes a block per wave.
//     A launch wants at least SPDP_FINDS_MIN_WAVES areas inside SPDP_FINDS_SLAB_BUDGET, so the slab serves a database of at most
//     SPDP_FINDS_MAX_BLOCKS blocks (one block per sequence in a -KA index) and is refused by name beyond;
//   * THE TABLE: S slots (a power of two) of 16 bytes, {block, tag} and {tag, value}, open-addressed and keyed by block
//     (spdp_blk_finds.h, "score slots") -- a probe and a compare-and-swap for a block's first entry, a probe, a load and a store for
//     the later ones.  The area is a header, the table, the staging list and the run hash when LDS has no room for it: NOTHING IN IT
//     GROWS WITH nseg (lenadj stays one array for all waves).  A query whose blocks fill the table ends at once, writes no record
//     and puts its number on the launch's list (BlkFindsArgs::over, counted in next[1]); the host reads the counter and the word beside it, the
//     most blocks a query scored -- 8 bytes, all there is to read when nothing overflowed --, runs the listed queries again on tables of 4 S slots (BlkFindsArgs::which), and so on until the list
//     is empty.  A table of at least nseg + 1 slots cannot fill (the probe visits every slot, a block number is below nseg).
// SPDP_FINDS_RSCR=slab|hash in the environment when an index is first searched chooses; unset: the slab up to
// SPDP_FINDS_MAX_BLOCKS blocks, the table beyond.  SPDP_FINDS_RSCR_SLOTS=<n> sets the first S (rounded up to a power of two, at
// least 64; default SPDP_FINDS_TABLE_SLOTS).  Both forms measured side by side: MEASUREMENTS.md, "Protein database search".
#define SPDP_FINDS_SLAB_BUDGET ((size_t) 8 << 30)
#define SPDP_FINDS_MIN_WAVES 64
#define SPDP_FINDS_MAX_BLOCKS (1 << 24)
#define SPDP_FINDS_TABLE_SLOTS (1u << 15)
#define SPDP_FINDS_TABLE_MIN_SLOTS 64u
#define SPDP_FINDS_HH_LDS_BYTES (24u << 10)     // the run hash lives in LDS up to this size (six waves a CU), in the slab beyond

struct BlkFindsArgs {
    const BlkDev* ix;                           // in device memory
    const int32_t* lenadj; int64_t n_words;
    int32_t max_out, ptpl, maxmmc;
    const uint8_t* codes; const int64_t* offs; const int32_t* left; const int32_t* right;
    int32_t* out; int out_cap, n;
    uint8_t* slabs; size_t slab_bytes;          // one area per wave of the launch; zero when allocated, kept between launches
    uint32_t* next;                             // four words the launch clears: [0] its query counter, [1] the queries on `over`,
                                                // [2] the most distinct blocks one query scored (table form)
    uint32_t tb_n;                              // 0: the slab form; else the slots of a wave's table, a power of two
    const int32_t* which;                       // null: queries 0 .. n - 1; else the n queries to run
    int32_t* over;                              // table form: room for n query numbers
    int n_waves, hh_n, hh_step, hh_in_lds;
    uint32_t lds_bytes;
};
#ifdef __HIPCC__
extern "C" hipError_t spdp_blk_finds_launch(const BlkFindsArgs* a, hipStream_t s);
#endif
extern "C" size_t spdp_blk_finds_area_bytes(const BlkDev* ix, int hh_n, int hh_in_lds, uint32_t tb_n);      // tb_n = 0: the slab form
extern "C" uint32_t spdp_blk_finds_lds_bytes(const BlkDev* ix, int hh_n, int hh_in_lds);

// the resident index as the finds entries see it (spdp_blk_api.cpp): its context, the index as the kernels read it (host view and
// device copy), and a place for what the finds vote keeps with the index between calls (freed with it)
struct SpdpBlkIndex;
struct SpdpContext;
struct BlkFindsKept { virtual ~BlkFindsKept() {} };
SpdpContext* spdp_blk_index_ctx(const SpdpBlkIndex* ix);
const BlkDev* spdp_blk_index_view(const SpdpBlkIndex* ix);
const BlkDev* spdp_blk_index_on_device(SpdpBlkIndex* ix);      // null: see the context's error
BlkFindsKept*& spdp_blk_index_finds_kept(SpdpBlkIndex* ix);
int64_t spdp_blk_index_n_words(const SpdpBlkIndex* ix);       // entries of blkb on the device
#endif
