// spdp_blk_finds.h -- the vote of SrchBlk::finds (protein query x protein database, ogotoh/spaln v3.0.7 src/blksrc.cc:3271-3362
// with init2 :1925-1938, Bhit2 :3147-3179, Randbs :2047-2069, findChrNo :1985-2002, the one-argument Qwords::querywords
// :2836-2878 and the merged posting lists :2938-2969) as ONE WAVE works it, in plain C++ that compiles twice:
//   * with SPDP_FINDS_DEVICE defined (spdp_blk_finds.hip) every function is device code, a per-lane value is a register and a
//     "for each lane" block is the lane itself;
//   * without it (tests/finds_host_check.cpp) a per-lane value is an array of 64, a "for each lane" block is a loop, a ballot
//     is a loop -- the same statements in the same order, one phase after the other, on the CPU under the sanitizers.
// Between two phases that hand data from lane to lane stands finds_sync() (a wave barrier on the device, nothing on the host);
// inside a phase no lane reads what another lane writes in the same phase.
//
// The layout for the machine is the one of the findblock vote (spdp_blk_vote.hip): control flow -- rounds, the two directions,
// the Nshift phases, the end of a run -- is uniform per query; the data of a step is a posting list spread over the 64 lanes; the
// run hash keeps the reference's slot geometry (Dhash<INT,int>(2 MaxBlk, 0): home key % size1, stride size2 - key % size2, a
// block that fails to continue is written EMPTY, which cuts the probe chains that ran over it -- results depend on it), its 64
// updates of a chunk decided on a snapshot and committed up to the first lane whose probe path meets a lower lane's write; the
// scores rscr[block] are {query tag, value} slots, never cleared, in one of two stores (FindsWave::store): the wave's slab of
// nseg + 1 slots, a block's slot at its number, or an open-addressed table of tb_n slots keyed by block ("score slots" below);
// the Ncand heap sits in LDS, offers are decided in parallel and applied lowest lane first.
#ifndef SPDP_BLK_FINDS_H_
#define SPDP_BLK_FINDS_H_
#include <stdint.h>
#include <stddef.h>
#include <math.h>
#include "spdp_blk_dev.h"

#define SPDP_FINDS_SHORT 16             // = SPDP_BLK_SHORT (include/spdp.h): the query is shorter than Nshift + width, finds returns ERROR
#define SPDP_FINDS_OWN 256              // owner marks, slot number folded (a false meeting only splits a chunk early)
#define SPDP_FINDS_MAX_QUERY 65535      // a run counts its words in 16 bits beside the run's epoch

#ifdef SPDP_FINDS_DEVICE
#define FD __device__ __forceinline__
#define EACH_LANE(l) for (int l = (int) threadIdx.x, once_ = 1; once_; once_ = 0)
template <class T> struct PerLane { T v; FD T& operator[](int) { return v; } FD const T& operator[](int) const { return v; } };
FD uint64_t finds_ballot(const PerLane<int>& p) { return __ballot(p.v != 0); }
FD void finds_sync() { wave_sync(); }
FD void finds_own_min(uint32_t* p, uint32_t v) { atomicMin(p, v); }
FD int finds_uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
// slots other lanes of the wave write: read and written past the L1, as the findblock vote does
FD uint64_t finds_ld(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
FD void finds_st(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// a slot several lanes may want at once: *p becomes `now` if it still holds `was` (-> 1), else it is left alone (-> 0)
FD int finds_cas(uint64_t* p, uint64_t was, uint64_t now)
{
    return __hip_atomic_compare_exchange_strong(p, &was, now, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
FD int finds_first(uint64_t m) { return __ffsll((long long) m) - 1; }
FD int finds_popc(uint64_t m) { return __popcll(m); }
#else
#define FD inline
#define EACH_LANE(l) for (int l = 0; l < 64; ++l)
template <class T> struct PerLane { T v[64]; T& operator[](int l) { return v[l]; } const T& operator[](int l) const { return v[l]; } };
inline uint64_t finds_ballot(const PerLane<int>& p) { uint64_t m = 0; for (int l = 0; l < 64; ++l) if (p.v[l]) m |= 1ull << l; return m; }
inline void finds_sync() {}
inline void finds_own_min(uint32_t* p, uint32_t v) { if (v < *p) *p = v; }
inline int finds_uni(int x) { return x; }
inline uint64_t finds_ld(const uint64_t* p) { return *p; }
inline void finds_st(uint64_t* p, uint64_t v) { *p = v; }
inline int finds_cas(uint64_t* p, uint64_t was, uint64_t now) { if (*p != was) return 0; *p = now; return 1; }      // (one lane after the other: a plain compare and store)
inline int finds_first(uint64_t m) { return __builtin_ffsll((long long) m) - 1; }
inline int finds_popc(uint64_t m) { return __builtin_popcountll(m); }
#endif

enum { FST_FRONT = 0, FST_TROUBLE = 1, FST_TW0 = 2, FST_TW1 = 3, FST_STAGED = 4, FST_FULL = 5, FST_WORDS = 8 };

// what a wave works with.  LDS: st, as, own, heap (and hh when it fits); the wave's area of HBM: rscr or tb, stage (and hh when
// it does not)
struct FindsWave {
    const BlkDev* X;
    const int32_t* lenadj;              // per block Randbs::lencor(SegLen[blk]) (setSegLen :1966-1983), nseg + 1 of them
    int64_t n_words;                    // entries of blkb
    int32_t max_out, ptpl, maxmmc;      // OutPrm.MaxOut; ptpl = base() / AvrScr (:2211); maxmmc (:2207: INT_MAX for a local search)
    int* st; int* as; uint32_t* own;
    uint64_t* heap;                     // {block, score}: block << 32 | score; ncand + 1 of them
    uint64_t* hh; uint32_t hh_n, hh_step, epoch;        // the run hash: key << 32 | epoch << 16 | count
    uint64_t* rscr; uint32_t tag;       // tag << 32 | value
    uint32_t* stage;                    // two posting lists merged (2 maxlist + 2)
    int store = 0;                      // what holds the scores: 0 the slab rscr, 1 the table tb
    uint64_t* tb = nullptr;             // tb_n slots of two words: block << 32 | tag, tag << 32 | value
    uint32_t tb_n = 0, tb_shift = 0;    // a power of two, and 32 - its logarithm
    int n_scored = 0;                   // the distinct blocks the query has scored so far (counted in the table form only)
};

FD uint32_t finds_no_lane() { return 0xffffffffu; }

// ---- Randbs::randbs
FD int finds_randbs(const BlkDev& X, uint32_t mmc)
{
    if (mmc < 128) return X.rscrtab[mmc];
    if (X.rbscoef == 0) return (int) X.rbscons;
    const double x = (double) (mmc + 1);
    return (int) (X.rbscoef * (X.gdb ? log(x) : sqrt(x)) + X.rbscons);
}

// ---- SrchBlk::findChrNo: the bracket of the linear estimate decides ties of equal first blocks, so it is kept
FD uint32_t finds_first_block(const BlkDev& X, int c) { return (uint32_t) X.chr[2 * c + 1]; }
FD int finds_chr_of(const BlkDev& X, uint32_t blk)
{
    int lo = (int) (X.bclw + X.bcce * (blk - 1)) - 1, hi = (int) (X.bcup + X.bcce * (blk - 1)) + 1;
    if (lo < 0) lo = 0;
    if (lo > X.n_chr) lo = X.n_chr;     // (a malformed Block2Chr: the table has n_chr + 1 entries)
    if (hi > X.n_chr) hi = X.n_chr;
    if (hi < 0) hi = 0;
    if (finds_first_block(X, lo) > blk) lo = 0;
    if (finds_first_block(X, hi) < blk) hi = X.n_chr;
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (finds_first_block(X, mid) > blk) hi = mid;
        else if (finds_first_block(X, mid + 1) > blk) return mid;
        else lo = mid;
    }
    return finds_first_block(X, hi) > blk ? lo : hi;
}

// ---- the words of the query (Qwords::querywords(ss), init_mrglist): score < 0 no usable word, 0 a ubiquitous one; the posting
// lists that vote (patterns 0 .. kk - 2; the only pattern when kk = 1)
struct FindsWord { int score; uint32_t off0, off1; int len0, len1; };

FD uint32_t finds_residue(const BlkDev& X, const uint8_t* q, int q_len, int i)
{
    if (i < 0 || i >= q_len) return 255u;
    const int c = q[i];
    return c < X.convts ? X.convtab[c] : 255u;
}
FD uint32_t finds_spell(const BlkDev& X, const uint8_t* q, int q_len, int ss, int k, int& good)
{
    const int32_t* bp = X.bitpat + X.pat_off[k];
    const int weight = bp[0];
    uint32_t w = 0;
    int i = 0;
    for ( ; i < weight; ++i) {
        const uint32_t c = finds_residue(X, q, q_len, ss + bp[3 + i]);
        if (c >= (uint32_t) X.nalpha) break;
        w = w * (uint32_t) X.nalpha + c;
    }
    good = i;
    return w;
}
// a list as the kernel may read it: inside blkb, no longer than the index's longest
FD void finds_list(const FindsWave& W, uint32_t x, int32_t lp, uint32_t& off, int& len)
{
    off = (uint32_t) lp - 1u; len = W.X->nblk[x];
    if (len > W.X->maxlist) len = W.X->maxlist;
    if (lp < 1 || (int64_t) off + len > W.n_words) { off = 0; len = 0; W.st[FST_TROUBLE] |= 4; }       // SPDP_BLK_TABLE
}
FD FindsWord finds_word(const FindsWave& W, const uint8_t* q, int q_len, int right, int ss)
{
    const BlkDev& X = *W.X;
    FindsWord w; w.score = -1; w.off0 = w.off1 = 0; w.len0 = w.len1 = 0;
    const uint32_t tab = (uint32_t) X.tabsize;
    if (X.kk == 1) {
        int good;
        const uint32_t x = finds_spell(X, q, q_len, ss, 0, good);
        if (x >= tab) return w;
        const int32_t lp = X.blkp[x];
        if (!lp) { w.score = 0; return w; }             // (asked before the word is known to be whole, as the reference does)
        if (good != X.bitpat[X.pat_off[0]]) return w;
        w.score = X.wscr[x];
        if (w.score > 0) finds_list(W, x, lp, w.off0, w.len0);
        return w;
    }
    int n_ok = 0, sum = 0;
    for (int k = 0; k < X.kk; ++k) {
        const int32_t* bp = X.bitpat + X.pat_off[k];
        if (ss >= right - bp[1]) break;                 // (no room for this pattern, nor for the later ones)
        int good;
        const uint32_t x = finds_spell(X, q, q_len, ss, k, good);
        if (x >= tab || X.wscr[x] < 0 || good < bp[0]) continue;
        const int32_t lp = X.blkp[x];
        if (!lp) continue;
        ++n_ok; sum += X.wscr[x];
        if (k == 0) finds_list(W, x, lp, w.off0, w.len0);
        else if (k == 1 && X.kk > 2) finds_list(W, x, lp, w.off1, w.len1);      // (the last pattern scores but does not vote)
    }
    if (n_ok) w.score = (int) ((double) sum / X.app_c);
    return w;
}

// ---- score slots.  A value is {query tag, value}: a slot of an earlier query reads as 0 and nothing is cleared between queries.
// The slab: the slot of a block is at its number.  The table: a slot is two words, {block, tag} and {tag, value}; a block's slot is
// the first of its probe sequence (home = the block's multiplicative hash, then the next slot, round the table) that holds the
// block under this query's tag, or the first that holds no block of this query, which the lane claims with finds_cas -- the lanes
// of a chunk insert at the same time and may want the same free slot; the loser reads the slot again, finds this query's tag in it
// and walks on.  UNLIKE THE RUN HASH, NO RESULT DEPENDS ON THE SLOT GEOMETRY: a block's value is only read, increased and written
// back, nothing is ever emptied, so any table size and any probe that visits every slot give the same records.  A block twice in
// one chunk (a malformed index): both lanes end on one slot, each adds to what it read, one store stays -- as in the slab.
// get -> the value, `at`: where put writes it, finds_no_lane() when the probe went round a table full of this query's blocks;
// fresh: the block had no slot in this query yet and this lane made it one
FD int finds_rscr_value(const FindsWave& W, uint64_t x) { return (uint32_t) (x >> 32) == W.tag ? (int) (uint32_t) x : 0; }
FD int finds_rscr_get(const FindsWave& W, uint32_t blk, uint32_t& at, int& fresh)
{
    fresh = 0;
    if (!W.store) { at = blk; return finds_rscr_value(W, finds_ld(W.rscr + blk)); }
    const uint64_t mine = ((uint64_t) blk << 32) | W.tag;
    uint32_t s = (blk * 0x9e3779b1u) >> W.tb_shift;
    for (uint32_t seen = 0; seen < W.tb_n; ) {
        uint64_t* slot = W.tb + 2 * (size_t) s;
        const uint64_t k = finds_ld(slot);
        if (k == mine) { at = s; return finds_rscr_value(W, finds_ld(slot + 1)); }
        if ((uint32_t) k == W.tag) { s = (s + 1) & (W.tb_n - 1); ++seen; continue; }    // another block of this query
        if (finds_cas(slot, k, mine)) { at = s; fresh = 1; return 0; }                  // (its value word is an earlier query's: 0)
        // lost to another lane: the slot now carries this query's tag and is not free again, so it is read once more, not for ever
    }
    at = finds_no_lane();
    return 0;
}
FD void finds_rscr_put(const FindsWave& W, uint32_t at, int v)
{
    finds_st(W.store ? W.tb + 2 * (size_t) at + 1 : W.rscr + at, ((uint64_t) W.tag << 32) | (uint32_t) v);
}

// ---- the run hash
FD uint32_t finds_hh_key(uint64_t s) { return (uint32_t) (s >> 32); }
FD int finds_hh_count(const FindsWave& W, uint64_t s) { const uint32_t v = (uint32_t) s; return (v >> 16) == W.epoch ? (int) (v & 0xffffu) : 0; }
FD void finds_hh_put(const FindsWave& W, uint32_t slot, uint32_t key, int count)
{
    finds_st(W.hh + slot, ((uint64_t) key << 32) | (W.epoch << 16) | (uint32_t) (count & 0xffff));
}
FD void finds_new_run(FindsWave& W)                     // hh.clear(): all lanes, uniform
{
    if (++W.epoch < 65536u) return;
    EACH_LANE(l) for (uint32_t i = (uint32_t) l; i < W.hh_n; i += 64) finds_st(W.hh + i, 0);
    W.epoch = 1;
    finds_sync();
}
// Dhash::map on the table as it stands: the first slot of the key's probe sequence that is empty or its own.  round: the probe
// came back to its home (the reference grows the table there; a list no longer than MaxBlk never gets that far)
FD uint32_t finds_place(const FindsWave& W, uint32_t key, int& count, int& round)
{
    uint32_t s = key % W.hh_n;
    const uint32_t u = W.hh_step - key % W.hh_step, s0 = s;
    round = 0;
    for (;;) {
        const uint64_t kv = finds_ld(W.hh + s);
        count = finds_hh_count(W, kv);
        if (!count || finds_hh_key(kv) == key) return s;
        s = (s + u) % W.hh_n;
        if (s == s0) { round = 1; count = 0; return s; }
    }
}
// the same walk, asking the owner marks: does a lower lane empty or claim a slot this lane reads?
FD int finds_path_meets_lower(const FindsWave& W, uint32_t key, uint32_t me)
{
    uint32_t s = key % W.hh_n;
    const uint32_t u = W.hh_step - key % W.hh_step, s0 = s;
    for (;;) {
        if (W.own[s & (SPDP_FINDS_OWN - 1)] < me) return 1;
        const uint64_t kv = finds_ld(W.hh + s);
        if (!finds_hh_count(W, kv) || finds_hh_key(kv) == key) return 0;
        s = (s + u) % W.hh_n;
        if (s == s0) return 0;
    }
}

// ---- the Ncand heap: PrQueue<BlkScr>(blkscr, Ncand, 0, false, true) (src/clib.h:446-565) -- a min-heap by score, a block found
// by looking at every entry (find), put(x, p) replacing entry p (or the top when the heap is full) if x scores higher
FD uint32_t finds_hp_key(uint64_t e) { return (uint32_t) (e >> 32); }
FD int finds_hp_val(uint64_t e) { return (int) (uint32_t) e; }
FD uint64_t finds_hp(uint32_t key, int val) { return ((uint64_t) key << 32) | (uint32_t) val; }
FD void finds_downheap(uint64_t* data, int k, int kmax)
{
    const uint64_t v = data[k];
    while (k < kmax / 2) {
        int c = 2 * k + 1;
        if (c + 1 < kmax && finds_hp_val(data[c + 1]) < finds_hp_val(data[c])) ++c;
        if (!(finds_hp_val(data[c]) < finds_hp_val(v))) break;
        data[k] = data[c];
        k = c;
    }
    data[k] = v;
}
FD void finds_upheap(uint64_t* data, int k)
{
    const uint64_t v = data[k];
    int h = (k - 1) / 2;
    while (k && finds_hp_val(v) < finds_hp_val(data[h])) { data[k] = data[h]; k = h; h = (h - 1) / 2; }
    data[k] = v;
}
FD int finds_heap_find(const FindsWave& W, uint32_t key)
{
    const int n = W.st[FST_FRONT];
    for (int i = 0; i < n; ++i) if (finds_hp_key(W.heap[i]) == key) return i;
    return -1;
}
FD int finds_offer_matters(const FindsWave& W, uint32_t key, int score)
{
    const int at = finds_heap_find(W, key);
    if (at < 0 && W.st[FST_FRONT] < W.X->ncand) return 1;
    return finds_hp_val(W.heap[at < 0 ? 0 : at]) < score;
}
FD void finds_offer(const FindsWave& W, uint32_t key, int score)        // Bhit2::update, one lane
{
    int at = finds_heap_find(W, key);
    if (at < 0) {
        if (W.st[FST_FRONT] < W.X->ncand) { const int k = W.st[FST_FRONT]++; W.heap[k] = finds_hp(key, score); finds_upheap(W.heap, k); return; }
        at = 0;
    }
    if (finds_hp_val(W.heap[at]) < score) { W.heap[at] = finds_hp(key, score); finds_downheap(W.heap, at, W.st[FST_FRONT]); }
}
// the offers of the lanes in `who`, in lane order: those that would change nothing are skipped, the heap read again after each
FD void finds_offer_in_order(const FindsWave& W, uint64_t who, const PerLane<uint32_t>& key, const PerLane<int>& score)
{
    int from = 0;
    for (;;) {
        PerLane<int> mine;
        EACH_LANE(l) mine[l] = ((who >> l) & 1) && l >= from && finds_offer_matters(W, key[l], score[l]);
        const uint64_t m = finds_ballot(mine);
        if (!m) break;
        const int f = finds_first(m);
        EACH_LANE(l) if (l == f) finds_offer(W, key[l], score[l]);
        finds_sync();
        from = f + 1;
    }
}

// ---- the posting entries of a word: one list where it lies, two merged into the staging area by one lane (ascending, a block
// of both once; a zero ends the list it stands in, as a front of 0 does in Qwords::next_mrglist)
FD const uint32_t* finds_entries(const FindsWave& W, const FindsWord& w, int& n)
{
    const BlkDev& X = *W.X;
    if (!w.len1) { n = w.len0; return X.blkb + w.off0; }
    if (!w.len0) { n = w.len1; return X.blkb + w.off1; }
    EACH_LANE(l) if (l == 0) {
        const uint32_t* a = X.blkb + w.off0; const uint32_t* b = X.blkb + w.off1;
        int na = w.len0, nb = w.len1, i = 0, j = 0, k = 0;
        for (;;) {
            if (i < na && !a[i]) na = i;                // (a zero ends the list it stands in; the other goes on)
            if (j < nb && !b[j]) nb = j;
            if (i >= na && j >= nb) break;
            const uint32_t x = i < na ? a[i] : 0xffffffffu, y = j < nb ? b[j] : 0xffffffffu;
            const uint32_t m = x < y ? x : y;
            W.stage[k++] = m;
            i += x == m; j += y == m;
        }
        W.st[FST_STAGED] = k;
    }
    finds_sync();
    n = finds_uni(W.st[FST_STAGED]);
    return W.stage;
}

// One word, the p-th of its run: all its posting entries.  -> in how many blocks the run went on (q of SrchBlk::finds)
FD int finds_vote(FindsWave& W, const FindsWord& w, int p, int threshold)
{
    const BlkDev& X = *W.X;
    int n_all;
    const uint32_t* list = finds_entries(W, w, n_all);
    int went_on = 0;
    for (int c0 = 0; c0 < n_all; c0 += 64) {
        PerLane<uint32_t> blk; PerLane<int> have, flag;
        EACH_LANE(l) { have[l] = c0 + l < n_all; blk[l] = have[l] ? list[c0 + l] : 0u; flag[l] = have[l] && blk[l] == 0; }
        const uint64_t zeros = finds_ballot(flag);
        if (zeros) { const int cut = finds_first(zeros); EACH_LANE(l) have[l] = have[l] && l < cut; n_all = 0; }      // a zero ends the list
        EACH_LANE(l) flag[l] = have[l] && blk[l] >= (uint32_t) X.nseg;
        if (finds_ballot(flag)) {                       // (a block the slab has no slot for: a malformed index)
            EACH_LANE(l) { if (flag[l]) W.st[FST_TROUBLE] |= 4; have[l] = have[l] && !flag[l]; }
        }
        uint64_t pend = finds_ballot(have);
        while (pend) {
            PerLane<uint32_t> slot; PerLane<int> cur, ok, writes, meets, sig, run, fresh;
            EACH_LANE(l) {
                slot[l] = 0; cur[l] = 0; ok[l] = 0; writes[l] = 0;
                if ((pend >> l) & 1) {
                    int round;
                    slot[l] = finds_place(W, blk[l], cur[l], round);
                    if (round) W.st[FST_TROUBLE] |= 4;
                    ok[l] = cur[l] + 1 == p;
                    // what changes the table for a later lane's probe: a slot claimed (p = 1), a slot written empty
                    writes[l] = !round && (ok[l] ? cur[l] == 0 : cur[l] > 0);
                    if (writes[l]) finds_own_min(&W.own[slot[l] & (SPDP_FINDS_OWN - 1)], (uint32_t) l);
                    if (round) ok[l] = 0;
                }
            }
            finds_sync();
            EACH_LANE(l) meets[l] = ((pend >> l) & 1) && finds_path_meets_lower(W, blk[l], (uint32_t) l);
            const uint64_t met = finds_ballot(meets);
            finds_sync();
            EACH_LANE(l) if (writes[l]) W.own[slot[l] & (SPDP_FINDS_OWN - 1)] = finds_no_lane();
            const uint64_t go = pend & (met ? ((1ull << finds_first(met)) - 1) : ~0ull);
            EACH_LANE(l) {
                sig[l] = 0; run[l] = 0; fresh[l] = 0;
                if ((go >> l) & 1) {
                    if (ok[l]) {
                        finds_hh_put(W, slot[l], blk[l], p);
                        uint32_t at;
                        run[l] = finds_rscr_get(W, blk[l], at, fresh[l]) + w.score;
                        if (at == finds_no_lane()) W.st[FST_FULL] = 1;
                        else {
                            finds_rscr_put(W, at, run[l]);
                            sig[l] = run[l] >= threshold + W.lenadj[blk[l]];
                        }
                    } else if (cur[l] > 0) finds_hh_put(W, slot[l], blk[l], 0);
                } else ok[l] = 0;
            }
            finds_sync();
            went_on += finds_popc(finds_ballot(ok));
            if (W.store) {
                W.n_scored += finds_popc(finds_ballot(fresh));
                if (finds_uni(W.st[FST_FULL])) return went_on;              // the table is full: the query is over (finds_query)
            }
            const uint64_t sigm = finds_ballot(sig);
            if (sigm) finds_offer_in_order(W, sigm, blk, run);
            pend &= ~go;                                // (the lowest pending lane meets nobody: every turn commits at least one)
        }
    }
    return went_on;
}

// SrchBlk::finds for one query.  -> 1: the score table ran full; the query ended there, NOTHING was written to out and the caller
// runs it again on a larger table (0 otherwise, and always with the slab).  The record: [0] ints used, [1] nmmc the scan ended in, [2] flags (SPDP_BLK_REACHED: searched;
// SPDP_BLK_SHORT: refused, nothing follows; SPDP_BLK_CUT; SPDP_BLK_TABLE), [3] [4] testword, [5] sigm, (block, score) x sigm in
// hsort order, n_cand, the candidate sequences (-1 - c for a sequence seen before: its slot keeps what it held)
FD int finds_query(FindsWave& W, const uint8_t* q, int q_len, int left, int right, int32_t* out, int out_cap)
{
    const BlkDev& X = *W.X;
    const int nshift = X.nshift, width0 = X.bitpat[X.pat_off[0] + 1];
    const int qlen = right - left;
    EACH_LANE(l) if (l < FST_WORDS) W.st[l] = 0;
    W.n_scored = 0;
    finds_sync();
    if (qlen - (nshift + width0) < 1 || nshift > SPDP_BLK_MAX_SHIFT || qlen > SPDP_FINDS_MAX_QUERY) {
        EACH_LANE(l) if (l == 0) { if (out_cap > 0) out[0] = out_cap < 3 ? out_cap : 3; if (out_cap > 1) out[1] = 0; if (out_cap > 2) out[2] = SPDP_FINDS_SHORT; }
        return 0;
    }
    // init2: Nshift consecutive start points at the left end, the last Nshift whole words at the right end, the phase of a
    // right-end point chosen so that the two ends of a phase are a multiple of Nshift apart
    const int ts = right - (width0 + nshift) + 1;
    EACH_LANE(l) if (l < nshift) {
        W.as[l] = left + l;
        W.as[32 + ((ts - left) % nshift + l) % nshift] = ts + l;
    }
    finds_sync();
    const int c = qlen / (2 * nshift) - 1;
    const int rms = right - nshift * (c < W.ptpl ? c : W.ptpl);
    const int base = X.rscrtab[0];
    int meet = 0, full = 0;
    uint32_t nmmc = 0;
    for ( ; nmmc < (uint32_t) W.maxmmc && !meet && !full; ++nmmc) {
        const int threshold = finds_randbs(X, nmmc);
        for (int d = 0; d < 2 && !full; ++d) {
            for (int s = 0; s < nshift && !full; ++s) {
                int ms = finds_uni(W.as[32 * (1 - d) + s]);
                if (ms > rms) ms = rms;
                int cscr = 0, p = 0, more = 0;
                finds_new_run(W);
                do {                                    // continuous hits
                    const int ss = finds_uni(W.as[32 * d + s]);
                    finds_sync();
                    EACH_LANE(l) if (l == 0) W.as[32 * d + s] = ss + (d ? -nshift : nshift);
                    finds_sync();
                    if (d ^ (ss >= ms)) { meet = 1; break; }            // has scanned
                    const FindsWord w = finds_word(W, q, q_len, right, ss);
                    if (w.score < 0) break;
                    EACH_LANE(l) if (l == 0) ++W.st[FST_TW0 + d];
                    if (w.score == 0) { more = 1; continue; }           // ubiquitous
                    ++p; cscr += w.score;
                    more = finds_vote(W, w, p, threshold);
                    if (W.store) full = finds_uni(W.st[FST_FULL]);
                } while (more && cscr < base && !full);
            }
        }
    }
    finds_sync();
    if (full) return 1;
    // hsort, the first min(MaxOut, sigm) blocks, findChrNo on each (one lane)
    EACH_LANE(l) if (l == 0) {
        const int sigm = W.st[FST_FRONT];
        for (int k = sigm; --k > 0; ) { const uint64_t t = W.heap[0]; W.heap[0] = W.heap[k]; W.heap[k] = t; finds_downheap(W.heap, 0, k); }
        int n = 6;
        auto put = [&](int v) { if (n < out_cap) out[n] = v; ++n; };
        for (int i = 0; i < sigm; ++i) { put((int) finds_hp_key(W.heap[i])); put(finds_hp_val(W.heap[i])); }
        const int w = W.max_out < sigm ? W.max_out : sigm;
        put(w);
        const int first_cand = n;
        for (int i = 0; i < w; ++i) {
            const int chr = finds_chr_of(X, finds_hp_key(W.heap[i]));
            bool seen = false;                          // (shash: at most MaxOut entries, looked through)
            for (int j = 0; j < i && !seen; ++j) if (first_cand + j < out_cap) { const int o = out[first_cand + j]; seen = (o < 0 ? -1 - o : o) == chr; }
            put(seen ? -1 - chr : chr);
        }
        int flags = 1 | (W.st[FST_TROUBLE] & 4);
        if (n > out_cap) flags |= 2;
        if (out_cap > 0) out[0] = n < out_cap ? n : out_cap;
        if (out_cap > 1) out[1] = (int) nmmc;
        if (out_cap > 2) out[2] = flags;
        if (out_cap > 3) out[3] = W.st[FST_TW0];
        if (out_cap > 4) out[4] = W.st[FST_TW1];
        if (out_cap > 5) out[5] = sigm;
    }
    finds_sync();
    return 0;
}
#endif
