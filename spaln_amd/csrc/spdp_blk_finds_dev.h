// spdp_blk_finds_dev.h -- what the finds vote's kernel (spdp_blk_finds.hip) and its host side (spdp_blk_finds_api.cpp) share, and
// what the host side asks of the resident index (spdp_blk_api.cpp).  Data only.
#ifndef SPDP_BLK_FINDS_DEV_H_
#define SPDP_BLK_FINDS_DEV_H_
#include "spdp_blk_dev.h"

// WHAT HOLDS rscr.  The reference keeps rscr[nseg] per thread and clears it per query.  Here a wave owns a slab of nseg + 1
// {query tag, value} slots in HBM (8 bytes a block): nothing is cleared between queries, and a posting entry costs one load and
// one store at an address its block number gives.  The other form -- a per-wave hash keyed by block, sized by the blocks a query
// touches -- would bound the memory by the query instead of the database; nobody has measured which of the two is faster, the
// slab was chosen because the genome vote has it and a probe sequence per posting entry is what the run hash already costs.
// Its limit: a launch wants at least SPDP_FINDS_MIN_WAVES slabs inside SPDP_FINDS_SLAB_BUDGET, so a database of more than
// SPDP_FINDS_MAX_BLOCKS blocks (one block per sequence in a -KA index) is refused by name.
#define SPDP_FINDS_SLAB_BUDGET ((size_t) 8 << 30)
#define SPDP_FINDS_MIN_WAVES 64
#define SPDP_FINDS_MAX_BLOCKS (1 << 24)
#define SPDP_FINDS_HH_LDS_BYTES (24u << 10)     // the run hash lives in LDS up to this size (six waves a CU), in the slab beyond

struct BlkFindsArgs {
    const BlkDev* ix;                           // in device memory
    const int32_t* lenadj; int64_t n_words;
    int32_t max_out, ptpl, maxmmc;
    const uint8_t* codes; const int64_t* offs; const int32_t* left; const int32_t* right;
    int32_t* out; int out_cap, n;
    uint8_t* slabs; size_t slab_bytes;          // one per wave of the launch; zero when allocated, kept between launches
    uint32_t* next;                             // the launch's query counter
    int n_waves, hh_n, hh_step, hh_in_lds;
    uint32_t lds_bytes;
};
#ifdef __HIPCC__
extern "C" hipError_t spdp_blk_finds_launch(const BlkFindsArgs* a, hipStream_t s);
#endif
extern "C" size_t spdp_blk_finds_slab_bytes(const BlkDev* ix, int hh_n, int hh_in_lds);
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
